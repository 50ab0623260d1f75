// gpca_logistic_null / gpca_assoc_logistic_score / gpca_normal_log10p (include/gpca.h section a13): the logistic score scan.  The
// null model of every trait is fitted on the host in f64 (Newton on the standardised design, at most 62 x 62 Cholesky per step) and
// reduced to Pc + 3 panel columns; a count kernel takes the exact per-row sums and with them the flip, one pass over the band's kept
// rows multiplies the panel on the matrix cores (k_assoc_score), a third kernel makes the statistics (k_assoc_score_finish).  The call
// has its own workspace, allocated and freed per call, and reads nothing of the handle's state but the genotypes and the kept rows.
// gpca_assoc_logistic_spa / gpca_spa_log10p (section a14): the same call with the saddle-point correction after the finish kernel
// (assoc_spa.hip: the items with |z| >= spa_z, flagged and computed in ranges of kAspListItems), and the correction for one given
// vector on the host; both run the rules of spa_math.h.
#include "gpca_internal.h"
#include "spa_math.h"

using namespace gpca;

namespace {
struct AsrWs {
    float* Bt = nullptr;
    unsigned *incw = nullptr, *sums = nullptr;
    double *dv = nullptr, *stats = nullptr, *ua = nullptr, *info = nullptr;
    unsigned long long* bad = nullptr;
    // the saddle-point correction's: Z and mu of the traits, the slices of g~, the list of a range and its counter, the results
    double *Z = nullptr, *mu = nullptr, *g = nullptr, *spa = nullptr;
    int* list = nullptr;
    unsigned* count = nullptr;
    ~AsrWs() {
        dfree(Bt); dfree(incw); dfree(sums); dfree(dv); dfree(stats); dfree(ua); dfree(info); dfree(bad);
        dfree(Z); dfree(mu); dfree(g); dfree(spa); dfree(list); dfree(count);
    }
};
template <typename T>
hipError_t dalloc(T*& p, size_t elems) { return hipMalloc((void**)&p, std::max<size_t>(elems, 1) * sizeof(T)); }

constexpr int kLogitMaxSteps = 25;
constexpr double kLogitStop = 1e-10, kLogitMaxEta = 30.0, kLogitPivot = 1e-10;

// The design shared by the traits of a call: S and X = (1, the columns of C centred over S and scaled to unit norm), column-major
// [Pc + 1][n] (asc_design's standardisation and its constant-column test).
struct LogitDesign {
    std::vector<int64_t> S;
    std::vector<double> X;
    int P = 0;                      // Pc + 1
};
int logit_design(const double* C, int Pc, const uint8_t* include, int64_t N, LogitDesign& D, std::string& msg) {
    D.S.clear();
    D.S.reserve((size_t)N);
    for (int64_t n = 0; n < N; ++n) if (!include || include[n]) D.S.push_back(n);
    const int64_t ns = (int64_t)D.S.size();
    D.P = Pc + 1;
    if (ns - Pc - 1 < 1) { msg = std::to_string(ns) + " included samples leave n - Pc - 1 < 1"; return GPCA_ERR_BAD_ARG; }
    D.X.assign((size_t)D.P * (size_t)ns, 1.0);
    for (int j = 0; j < Pc; ++j) {
        double* c = &D.X[(size_t)(j + 1) * (size_t)ns];
        double sum = 0.0, raw = 0.0, ss = 0.0;
        for (int64_t i = 0; i < ns; ++i) {
            c[i] = C[D.S[(size_t)i] * Pc + j];
            if (!std::isfinite(c[i])) { msg = "C[" + std::to_string(D.S[(size_t)i]) + "][" + std::to_string(j) + "] is not finite"; return GPCA_ERR_BAD_ARG; }
            sum += c[i]; raw += c[i] * c[i];
        }
        const double mean = sum / (double)ns;
        for (int64_t i = 0; i < ns; ++i) { c[i] -= mean; ss += c[i] * c[i]; }
        if (!std::isfinite(ss) || !(ss > 1e-20 * raw)) {
            msg = "column " + std::to_string(j) + " of C is constant over the included samples (or overflows)";
            return GPCA_ERR_BAD_ARG;
        }
        const double inv = 1.0 / std::sqrt(ss);
        for (int64_t i = 0; i < ns; ++i) c[i] *= inv;
    }
    return GPCA_OK;
}

// A = X^T diag(w) X = L L^T in place (lower triangle, row-major [P][P]); a pivot below kLogitPivot of its diagonal entry = collinear
int logit_cholesky(const LogitDesign& D, const std::vector<double>& w, std::vector<double>& A, std::string& msg) {
    const int P = D.P;
    const int64_t ns = (int64_t)D.S.size();
    A.assign((size_t)P * P, 0.0);
    for (int i = 0; i < P; ++i)
        for (int j = 0; j <= i; ++j) {
            const double *a = &D.X[(size_t)i * (size_t)ns], *b = &D.X[(size_t)j * (size_t)ns];
            double s = 0.0;
            for (int64_t n = 0; n < ns; ++n) s += w[(size_t)n] * a[n] * b[n];
            A[(size_t)i * P + j] = s;
        }
    for (int j = 0; j < P; ++j) {
        const double diag = A[(size_t)j * P + j];
        double d = diag;
        for (int k = 0; k < j; ++k) d -= A[(size_t)j * P + k] * A[(size_t)j * P + k];
        if (!(d > kLogitPivot * diag) || !std::isfinite(d)) {
            msg = "the covariates (1, C) are collinear over the included samples (Cholesky pivot " + std::to_string(j) + " failed)";
            return GPCA_ERR_BAD_ARG;
        }
        const double l = std::sqrt(d);
        A[(size_t)j * P + j] = l;
        for (int i = j + 1; i < P; ++i) {
            double s = A[(size_t)i * P + j];
            for (int k = 0; k < j; ++k) s -= A[(size_t)i * P + k] * A[(size_t)j * P + k];
            A[(size_t)i * P + j] = s / l;
        }
    }
    return GPCA_OK;
}

// eta = X alpha, mu = 1 / (1 + exp(-eta)) over S; false when some |eta| > kLogitMaxEta (or is not finite)
bool logit_mu(const LogitDesign& D, const std::vector<double>& alpha, std::vector<double>& mu) {
    const int64_t ns = (int64_t)D.S.size();
    bool ok = true;
    for (int64_t n = 0; n < ns; ++n) {
        double eta = 0.0;
        for (int j = 0; j < D.P; ++j) eta += D.X[(size_t)j * (size_t)ns + (size_t)n] * alpha[(size_t)j];
        if (!(std::fabs(eta) <= kLogitMaxEta)) ok = false;
        mu[(size_t)n] = 1.0 / (1.0 + std::exp(-eta));
    }
    return ok;
}

// Newton from alpha = (logit(ybar), 0, ...): (X^T W X) delta = X^T (y - mu) by Cholesky, alpha += delta, until max |delta| <=
// kLogitStop (1 + max |alpha|); mu over S is recomputed from the final alpha.  y: stride ys between samples.
int logit_null(const LogitDesign& D, const double* y, int64_t ys, std::vector<double>& alpha, std::vector<double>& mu, int& iters,
               std::string& msg) {
    const int P = D.P;
    const int64_t ns = (int64_t)D.S.size();
    std::vector<double> yv((size_t)ns);
    int64_t cases = 0;
    for (int64_t i = 0; i < ns; ++i) {
        const double v = y[D.S[(size_t)i] * ys];
        if (!(v == 0.0 || v == 1.0)) { msg = "y[" + std::to_string(D.S[(size_t)i]) + "] is neither 0 nor 1"; return GPCA_ERR_BAD_ARG; }
        yv[(size_t)i] = v;
        cases += v == 1.0;
    }
    if (cases == 0 || cases == ns) { msg = "only one class among the included samples"; return GPCA_ERR_BAD_ARG; }
    const double ybar = (double)cases / (double)ns;
    alpha.assign((size_t)P, 0.0);
    alpha[0] = std::log(ybar / (1.0 - ybar));
    mu.assign((size_t)ns, 0.0);
    std::vector<double> w((size_t)ns), A, g((size_t)P);
    iters = 0;
    bool done = false;
    for (int it = 0; it < kLogitMaxSteps && !done; ++it) {
        if (!logit_mu(D, alpha, mu)) { msg = "some |X alpha| exceeds 30 (separation)"; return GPCA_ERR_NOT_CONVERGED; }
        for (int64_t n = 0; n < ns; ++n) w[(size_t)n] = mu[(size_t)n] * (1.0 - mu[(size_t)n]);
        const int rc = logit_cholesky(D, w, A, msg);
        if (rc != GPCA_OK) return rc;
        for (int j = 0; j < P; ++j) {
            const double* x = &D.X[(size_t)j * (size_t)ns];
            double s = 0.0;
            for (int64_t n = 0; n < ns; ++n) s += x[n] * (yv[(size_t)n] - mu[(size_t)n]);
            g[(size_t)j] = s;
        }
        // L z = g, L^T delta = z
        for (int j = 0; j < P; ++j) {
            double s = g[(size_t)j];
            for (int k = 0; k < j; ++k) s -= A[(size_t)j * P + k] * g[(size_t)k];
            g[(size_t)j] = s / A[(size_t)j * P + j];
        }
        for (int j = P - 1; j >= 0; --j) {
            double s = g[(size_t)j];
            for (int k = j + 1; k < P; ++k) s -= A[(size_t)k * P + j] * g[(size_t)k];
            g[(size_t)j] = s / A[(size_t)j * P + j];
        }
        double dmax = 0.0, amax = 0.0;
        for (int j = 0; j < P; ++j) { alpha[(size_t)j] += g[(size_t)j]; dmax = std::max(dmax, std::fabs(g[(size_t)j])); }
        for (int j = 0; j < P; ++j) amax = std::max(amax, std::fabs(alpha[(size_t)j]));
        iters = it + 1;
        if (!std::isfinite(dmax) || !std::isfinite(amax)) { msg = "the Newton step is not finite"; return GPCA_ERR_NOT_CONVERGED; }
        done = dmax <= kLogitStop * (1.0 + amax);
    }
    if (!done) { msg = "no convergence after " + std::to_string(kLogitMaxSteps) + " Newton steps"; return GPCA_ERR_NOT_CONVERGED; }
    if (!logit_mu(D, alpha, mu)) { msg = "some |X alpha| exceeds 30 (separation)"; return GPCA_ERR_NOT_CONVERGED; }
    return GPCA_OK;
}

// the sums of spa_math.h over one given vector, in sample order
struct HostSpaEval {
    const double *g, *mu;
    int64_t n;
    void operator()(double tau, bool want0, double& k0, double& k1, double& k2) const {
#pragma clang fp contract(off)
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int64_t i = 0; i < n; ++i) {
            double t1, t2;
            spa_terms12(g[i], mu[i], tau, t1, t2);
            s1 = s1 + t1; s2 = s2 + t2;
            if (want0) s0 = s0 + spa_term0(g[i], mu[i], tau);
        }
        k0 = s0; k1 = s1; k2 = s2;
    }
};

// gpca_assoc_logistic_score (spa = nullptr) and gpca_assoc_logistic_spa: one path; the correction only adds to it
int assoc_logistic(gpca_handle* h, const std::string& f, const double* Y, int32_t T, const double* C, int32_t Pc, const uint8_t* include,
                   double max_vif, bool with_spa, double spa_z, int64_t row0, int64_t row1, double* stats, double* spa, double* ua,
                   double* rowinfo);
}  // namespace

extern "C" int gpca_logistic_null(const double* y, const double* C, int32_t Pc, const uint8_t* include, int64_t N, double* alpha,
                                  double* mu, int32_t* iters) {
    if (!y || N < 1 || Pc < 0 || (Pc > 0 && !C) || (!alpha && !mu)) return GPCA_ERR_BAD_ARG;
    LogitDesign D;
    std::string msg;
    int rc = logit_design(C, Pc, include, N, D, msg);
    if (rc != GPCA_OK) return rc;
    std::vector<double> a, m;
    int it = 0;
    rc = logit_null(D, y, 1, a, m, it, msg);
    if (iters) *iters = it;
    if (rc != GPCA_OK) return rc;
    if (alpha) for (int j = 0; j <= Pc; ++j) alpha[j] = a[(size_t)j];
    if (mu) {
        for (int64_t n = 0; n < N; ++n) mu[n] = 0.0;
        for (size_t i = 0; i < D.S.size(); ++i) mu[D.S[i]] = m[i];
    }
    return GPCA_OK;
}

extern "C" int gpca_assoc_logistic_score(gpca_handle* h, const double* Y, int32_t T, const double* C, int32_t Pc, const uint8_t* include,
                                         double max_vif, int64_t row0, int64_t row1, double* stats, double* ua, double* rowinfo) {
    if (!h) return GPCA_ERR_BAD_ARG;
    return assoc_logistic(h, "gpca_assoc_logistic_score", Y, T, C, Pc, include, max_vif, false, INFINITY, row0, row1, stats, nullptr, ua, rowinfo);
}

extern "C" int gpca_assoc_logistic_spa(gpca_handle* h, const double* Y, int32_t T, const double* C, int32_t Pc, const uint8_t* include,
                                       double max_vif, double spa_z, int64_t row0, int64_t row1, double* stats, double* spa, double* ua,
                                       double* rowinfo) {
    if (!h) return GPCA_ERR_BAD_ARG;
    return assoc_logistic(h, "gpca_assoc_logistic_spa", Y, T, C, Pc, include, max_vif, true, spa_z, row0, row1, stats, spa, ua, rowinfo);
}

namespace {
int assoc_logistic(gpca_handle* h, const std::string& f, const double* Y, int32_t T, const double* C, int32_t Pc, const uint8_t* include,
                   double max_vif, bool with_spa, double spa_z, int64_t row0, int64_t row1, double* stats, double* spa, double* ua,
                   double* rowinfo) {
    LOCK(h);
    if (!have_genotypes(h)) return fail(h, GPCA_ERR_STATE, f + ": no genotypes resident");
    if (h->sm.on)
        return fail(h, GPCA_ERR_STATE, f + ": the handle streams its matrix in panels, which is not implemented");
    if (multi_rank(h)) return fail(h, GPCA_ERR_STATE, f + ": the handle holds a shard of the rows, which is not implemented");
    if (!h->have_stats) return fail(h, GPCA_ERR_STATE, f + ": no standardisation: run gpca_snp_stats or gpca_set_standardization first");
    if (h->n_pca == 0) return fail(h, GPCA_ERR_STATE, f + ": no kept row (the keep mask is empty)");
    const int64_t K = h->n_pca, N = h->N;
    if (T < 1 || Pc < 0 || (int64_t)T * ((int64_t)Pc + 3) > kAsrMaxCols)
        return fail(h, GPCA_ERR_BAD_ARG, f + ": T >= 1, Pc >= 0 and T (Pc + 3) <= " + std::to_string(kAsrMaxCols) + " are required");
    if (!Y) return fail(h, GPCA_ERR_BAD_ARG, f + ": Y is required");
    if (Pc > 0 && !C) return fail(h, GPCA_ERR_BAD_ARG, f + ": C is required when Pc > 0");
    if (with_spa && !spa) return fail(h, GPCA_ERR_BAD_ARG, f + ": spa is required");
    if (!with_spa && !stats && !ua && !rowinfo) return fail(h, GPCA_ERR_BAD_ARG, f + ": stats, ua and rowinfo are all NULL");
    if (row0 < 0 || row1 < row0 || row1 > K)
        return fail(h, GPCA_ERR_BAD_ARG, f + ": rows must satisfy 0 <= row0 <= row1 <= K (K = " + std::to_string(K) + " kept rows)");
    if (!(max_vif >= 1.0) || !std::isfinite(max_vif)) return fail(h, GPCA_ERR_BAD_ARG, f + ": max_vif must be finite and at least 1");
    if (with_spa && !spa_z_ok(spa_z)) return fail(h, GPCA_ERR_BAD_ARG, f + ": spa_z must be at least 0.5, or +inf for no correction");
    if (N >= ((int64_t)1 << 30)) return fail(h, GPCA_ERR_BAD_ARG, f + ": 2^30 or more samples (the per-row sums are 32-bit)");
    const int L = asr_cols(T, Pc), P = Pc + 1;
    const int64_t npad = asc_npad(N);

    // host: the design, then per trait the null fit and its Pc + 3 columns
    LogitDesign D;
    std::string msg;
    int rc = logit_design(C, Pc, include, N, D, msg);
    if (rc != GPCA_OK) return fail(h, rc, f + ": " + msg);
    const int64_t ns = (int64_t)D.S.size();
    std::vector<float> Bt((size_t)asc_b_capacity(N, L), 0.0f);
    std::vector<unsigned> incw((size_t)asc_inc_capacity(N), 0u);
    for (int64_t n : D.S) incw[(size_t)(n >> 5)] |= 1u << (int)(n & 31);
    // (the correction's: Z_t = X L_t^-T and mu_t in f64, 0 outside S and past N; with spa_z = +inf no item is corrected: the flag
    // kernel alone runs, and the correction's inputs and workspace are neither built nor allocated)
    const bool correct = with_spa && std::isfinite(spa_z);
    const int64_t gpad = asp_gpad(N);
    std::vector<double> Zh(correct ? (size_t)asp_z_capacity(N, T, Pc) : 0, 0.0), muh(correct ? (size_t)asp_mu_capacity(N, T) : 0, 0.0);
    {
        std::vector<double> alpha, mu, w((size_t)ns), A, col((size_t)P * (size_t)ns), zc(correct ? (size_t)P * (size_t)ns : 0);
        for (int t = 0; t < T; ++t) {
            int it = 0;
            rc = logit_null(D, Y + t, T, alpha, mu, it, msg);
            if (rc != GPCA_OK) return fail(h, rc, f + ": trait " + std::to_string(t) + ": " + msg);
            for (int64_t i = 0; i < ns; ++i) w[(size_t)i] = mu[(size_t)i] * (1.0 - mu[(size_t)i]);
            rc = logit_cholesky(D, w, A, msg);
            if (rc != GPCA_OK) return fail(h, rc, f + ": trait " + std::to_string(t) + ": " + msg);
            // A L^T = W X, column by column: a_j = (w x_j - sum_{k < j} L_jk a_k) / L_jj
            for (int j = 0; j < P; ++j) {
                double* a = &col[(size_t)j * (size_t)ns];
                const double* x = &D.X[(size_t)j * (size_t)ns];
                for (int64_t i = 0; i < ns; ++i) a[i] = w[(size_t)i] * x[i];
                for (int k = 0; k < j; ++k) {
                    const double l = A[(size_t)j * P + k];
                    const double* ak = &col[(size_t)k * (size_t)ns];
                    for (int64_t i = 0; i < ns; ++i) a[i] -= l * ak[i];
                }
                const double inv = 1.0 / A[(size_t)j * P + j];
                for (int64_t i = 0; i < ns; ++i) a[i] *= inv;
            }
            for (int64_t i = 0; i < ns; ++i) {
                const size_t n = (size_t)D.S[(size_t)i];
                Bt[(size_t)asr_col_w(t) * (size_t)npad + n] = (float)w[(size_t)i];
                Bt[(size_t)asr_col_r(T, t) * (size_t)npad + n] = (float)(Y[(int64_t)n * T + t] - mu[(size_t)i]);
                for (int j = 0; j < P; ++j) Bt[(size_t)asr_col_a(T, Pc, t, j) * (size_t)npad + n] = (float)col[(size_t)j * (size_t)ns + (size_t)i];
            }
            if (!correct) continue;
            // Z L^T = X, column by column: z_j = (x_j - sum_{k < j} L_jk z_k) / L_jj
            for (int j = 0; j < P; ++j) {
                double* z = &zc[(size_t)j * (size_t)ns];
                const double* x = &D.X[(size_t)j * (size_t)ns];
                for (int64_t i = 0; i < ns; ++i) z[i] = x[i];
                for (int k = 0; k < j; ++k) {
                    const double l = A[(size_t)j * P + k];
                    const double* zk = &zc[(size_t)k * (size_t)ns];
                    for (int64_t i = 0; i < ns; ++i) z[i] -= l * zk[i];
                }
                const double inv = 1.0 / A[(size_t)j * P + j];
                for (int64_t i = 0; i < ns; ++i) z[i] *= inv;
            }
            for (int64_t i = 0; i < ns; ++i) {
                const size_t n = (size_t)D.S[(size_t)i];
                muh[(size_t)t * (size_t)gpad + n] = mu[(size_t)i];
                for (int j = 0; j < P; ++j) Zh[((size_t)t * P + (size_t)j) * (size_t)gpad + n] = zc[(size_t)j * (size_t)ns + (size_t)i];
            }
        }
    }
    const int64_t rows = row1 - row0;
    if (rows == 0) return GPCA_OK;
    const bool dstats = stats || with_spa;                      // (the flag kernel reads z from the device's stats)
    if (asr_count_blocks(rows) >= ((int64_t)1 << 31)) return fail(h, GPCA_ERR_BAD_ARG, f + ": the band makes 2^31 or more workgroups: ask for fewer rows");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->st));
    {
        const double need = 4.0 * (double)asc_b_capacity(N, L) + 4.0 * (double)asc_inc_capacity(N) + 8.0 * (double)asr_dv_capacity(rows, L) +
                            4.0 * (double)asr_sums_capacity(rows) + (dstats ? 8.0 * (double)asr_stats_capacity(rows, T) : 0.0) +
                            (with_spa ? 8.0 * (double)asp_out_capacity(rows, T) + 4.0 * (double)asp_list_capacity(rows, T) : 0.0) +
                            (correct ? 8.0 * (double)(asp_g_capacity(N) + asp_z_capacity(N, T, Pc) + asp_mu_capacity(N, T)) : 0.0) +
                            (ua ? 8.0 * (double)asr_ua_capacity(rows, T, Pc) : 0.0) + (rowinfo ? 8.0 * (double)asr_info_capacity(rows) : 0.0) +
                            (double)(64 << 20);
        size_t fr = 0, tot = 0;
        HIPCHK(hipMemGetInfo(&fr, &tot));
        if (need > (double)fr) {
            char buf[256];
            snprintf(buf, sizeof buf, "%s: the band needs %.3g GB of device memory, %.3g GB are free: ask for fewer rows", f.c_str(), need * 1e-9, (double)fr * 1e-9);
            return fail(h, GPCA_ERR_OOM, buf);
        }
    }
    const bool packed = h->storage == GPCA_STORE_2BIT;
    const void* G = packed ? (const void*)h->dG2 : (const void*)h->dG;
    const int64_t ldr = packed ? h->ld2 : h->ld8;
    hipStream_t st = h->st;
    AsrWs ws;
    HIPCHK(dalloc(ws.Bt, Bt.size())); HIPCHK(dalloc(ws.incw, incw.size())); HIPCHK(dalloc(ws.bad, 1));
    HIPCHK(dalloc(ws.dv, (size_t)asr_dv_capacity(rows, L))); HIPCHK(dalloc(ws.sums, (size_t)asr_sums_capacity(rows)));
    if (dstats) HIPCHK(dalloc(ws.stats, (size_t)asr_stats_capacity(rows, T)));
    if (ua) HIPCHK(dalloc(ws.ua, (size_t)asr_ua_capacity(rows, T, Pc)));
    if (rowinfo) HIPCHK(dalloc(ws.info, (size_t)asr_info_capacity(rows)));
    HIPCHK(hipMemcpyAsync(ws.Bt, Bt.data(), Bt.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ws.incw, incw.data(), incw.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(ws.bad, 0xff, 8, st));
    if (with_spa) {
        HIPCHK(dalloc(ws.spa, (size_t)asp_out_capacity(rows, T))); HIPCHK(dalloc(ws.list, (size_t)asp_list_capacity(rows, T)));
        HIPCHK(dalloc(ws.count, 1));
    }
    if (correct) {
        HIPCHK(dalloc(ws.Z, Zh.size())); HIPCHK(dalloc(ws.mu, muh.size())); HIPCHK(dalloc(ws.g, (size_t)asp_g_capacity(N)));
        HIPCHK(hipMemcpyAsync(ws.Z, Zh.data(), Zh.size() * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ws.mu, muh.data(), muh.size() * 8, hipMemcpyHostToDevice, st));
    }
    const double gbytes = (double)rows * (double)N * (packed ? 0.25 : 1.0);
    {
        ScopedTimer t(h, "assoc_score_count", 0.0, gbytes);
        if (launch_assoc_score_count(st, G, packed, ldr, h->d_pca_rows, N, ws.incw, row0, row1, ws.sums, ws.bad) != 0)
            return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
        HIPCHK(hipGetLastError());
    }
    {
        // flops as for k_assoc, the d product over the padded columns plus the q product over its one block
        ScopedTimer t(h, "assoc_score", 2.0 * (double)rows * (double)N * (double)(asc_lpad(L) + 32), gbytes);
        if (launch_assoc_score(st, G, packed, ldr, h->d_pca_rows, N, ws.Bt, ws.incw, T, L, row0, row1, ws.sums, ws.dv) != 0)
            return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
        HIPCHK(hipGetLastError());
    }
    launch_assoc_score_finish(st, ws.dv, ws.sums, T, Pc, max_vif, rows, ws.stats, ws.ua, ws.info);
    HIPCHK(hipGetLastError());
    if (with_spa) {
        ScopedTimer t(h, "assoc_spa", 0.0, 0.0);
        const int64_t items = rows * (int64_t)T;
        for (int64_t item0 = 0; item0 < items; item0 += kAspListItems) {
            HIPCHK(hipMemsetAsync(ws.count, 0, 4, st));
            launch_assoc_spa_flag(st, ws.stats, ws.dv, T, Pc, item0, std::min<int64_t>(kAspListItems, items - item0), spa_z, ws.spa, ws.list, ws.count);
            HIPCHK(hipGetLastError());
            if (!correct) continue;
            if (launch_assoc_spa(st, G, packed, ldr, h->d_pca_rows, N, ws.incw, ws.sums, ws.dv, ws.Z, ws.mu, T, Pc, row0, item0, ws.list, ws.count,
                                 ws.g, ws.spa) != 0)
                return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
            HIPCHK(hipGetLastError());
        }
    }
    unsigned long long bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, ws.bad, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (bad != ~0ull)
        return fail(h, GPCA_ERR_INVALID_GENOTYPE, f + ": row " + std::to_string(bad) + " holds a genotype outside {0, 1, 2, missing}");
    if (stats) HIPCHK(hipMemcpyAsync(stats, ws.stats, (size_t)asr_stats_capacity(rows, T) * 8, hipMemcpyDeviceToHost, st));
    if (ua) HIPCHK(hipMemcpyAsync(ua, ws.ua, (size_t)asr_ua_capacity(rows, T, Pc) * 8, hipMemcpyDeviceToHost, st));
    if (rowinfo) HIPCHK(hipMemcpyAsync(rowinfo, ws.info, (size_t)asr_info_capacity(rows) * 8, hipMemcpyDeviceToHost, st));
    if (with_spa) HIPCHK(hipMemcpyAsync(spa, ws.spa, (size_t)asp_out_capacity(rows, T) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GPCA_OK;
}
}  // namespace

extern "C" int gpca_spa_log10p(const double* gt, const double* mu, int64_t n, double u, double* log10p, double* zeta, int32_t* status) {
#pragma clang fp contract(off)
    if (!gt || !mu || n < 1 || !log10p || !std::isfinite(u)) return GPCA_ERR_BAD_ARG;
    double V = 0.0, hi = 0.0, lo = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        if (!std::isfinite(gt[i]) || !(mu[i] >= 0.0 && mu[i] <= 1.0)) return GPCA_ERR_BAD_ARG;
        double p, q;
        spa_support(gt[i], mu[i], p, q);
        hi = hi + p; lo = lo + q;
        V = V + (1.0 - mu[i]) * mu[i] * (gt[i] * gt[i]);
    }
    const HostSpaEval ev{gt, mu, n};
    SpaResult r;
    spa_item(ev, u, hi, lo, u == 0.0 ? 0.0 : spa_normal_log10p(u / std::sqrt(V)), r);
    *log10p = r.log10p;
    if (zeta) { zeta[0] = r.zeta[0]; zeta[1] = r.zeta[1]; }
    if (status) *status = r.status;
    return GPCA_OK;
}

// (spa_math.h holds the function: the kernels of assoc_spa.hip use it too)
extern "C" double gpca_normal_log10p(double z) { return spa_normal_log10p(z); }
