// gpca_logistic_null / gpca_assoc_logistic_score / gpca_normal_log10p (include/gpca.h section a13): the logistic score scan.  The
// null model of every trait is fitted on the host in f64 (Newton on the standardised design, at most 62 x 62 Cholesky per step) and
// reduced to Pc + 3 panel columns; a count kernel takes the exact per-row sums and with them the flip, one pass over the band's kept
// rows multiplies the panel on the matrix cores (k_assoc_score), a third kernel makes the statistics (k_assoc_score_finish).  The call
// has its own workspace, allocated and freed per call, and reads nothing of the handle's state but the genotypes and the kept rows.
// gpca_assoc_logistic_spa / gpca_spa_log10p (section a14): the same call with the saddle-point correction after the finish kernel
// (assoc_spa.hip: the items with |z| >= spa_z, flagged and computed in ranges of kAspListItems), and the correction for one given
// vector on the host; both run the rules of spa_math.h.
// gpca_assoc_logistic_firth / gpca_firth_log10p (section a15): the same call again with the approximate Firth correction in the
// saddle-point correction's place (assoc_firth.hip: the items with |z| >= firth_z, the same ranges, lists and inputs), and its host twin.
// What is here: the Newton fit, the per-trait panel columns, the two corrections' orchestration and the host-only entry points; the rest
// of the host front end is the linear scan's (gpca_assoc.cpp, declared in gpca_internal.h).
#include "gpca_internal.h"
#include "spa_math.h"

using namespace gpca;

namespace {
struct AsrWs {
    float* Bt = nullptr;
    unsigned *incw = nullptr, *sums = nullptr;
    double *dv = nullptr, *stats = nullptr, *ua = nullptr, *info = nullptr;
    unsigned long long* bad = nullptr;
    // a correction's (saddle-point or Firth): Z and mu of the traits, the slices of g~, the list of a range and its counter, the results
    double *Z = nullptr, *mu = nullptr, *g = nullptr, *corr = nullptr;
    int* list = nullptr;
    unsigned* count = nullptr;
    // a set call's: the listed rows' original rows, the strips of the sets' lower triangles, Phi
    int64_t* lrows = nullptr;
    AsgStrip* strips = nullptr;
    double* phi = nullptr;
    ~AsrWs() {
        dfree(Bt); dfree(incw); dfree(sums); dfree(dv); dfree(stats); dfree(ua); dfree(info); dfree(bad);
        dfree(Z); dfree(mu); dfree(g); dfree(corr); dfree(list); dfree(count); dfree(lrows); dfree(strips); dfree(phi);
    }
};

constexpr int kLogitMaxSteps = 25;
constexpr double kLogitStop = 1e-10, kLogitMaxEta = 30.0, kLogitPivot = 1e-10;

// The design shared by the traits of a call: S and X = (1, the columns of C centred over S and scaled to unit norm), column-major
// [Pc + 1][n] (the front end's standardisation and its constant-column test; incw as asc_sample_set leaves it).
struct LogitDesign {
    std::vector<int64_t> S;
    std::vector<double> X;
    int P = 0;                      // Pc + 1
};
int logit_design(const double* C, int Pc, const uint8_t* include, int64_t N, LogitDesign& D, std::vector<unsigned>* incw, std::string& msg) {
    asc_sample_set(include, N, D.S, incw);
    const int64_t ns = (int64_t)D.S.size();
    D.P = Pc + 1;
    if (ns - Pc - 1 < 1) { msg = std::to_string(ns) + " included samples leave n - Pc - 1 < 1"; return GPCA_ERR_BAD_ARG; }
    D.X.assign((size_t)D.P * (size_t)ns, 1.0);
    return asc_standardise(C, Pc, D.S, D.X.data() + ns, msg);
}

// A = X^T diag(w) X = L L^T (lower triangle, row-major [P][P]); a pivot below kLogitPivot of its diagonal entry = collinear
int logit_cholesky(const LogitDesign& D, const std::vector<double>& w, std::vector<double>& A, std::string& msg) {
    return asc_cholesky(D.X.data(), D.P, (int64_t)D.S.size(), w.data(), [](double d, double diag) { return d > kLogitPivot * diag && std::isfinite(d); },
                        A, msg);
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

// the sums of the Firth correction over one given vector, in sample order
struct HostFirthEval {
    const double *g, *mu;
    int64_t n;
    void operator()(double beta, double& k0, double& k1, double& k2, double& k3, double& k4) const {
#pragma clang fp contract(off)
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
        for (int64_t i = 0; i < n; ++i) {
            double t1, t2, t3, t4;
            firth_terms1234(g[i], mu[i], beta, t1, t2, t3, t4);
            s0 = s0 + spa_term0(g[i], mu[i], beta);
            s1 = s1 + t1; s2 = s2 + t2; s3 = s3 + t3; s4 = s4 + t4;
        }
        k0 = s0; k1 = s1; k2 = s2; k3 = s3; k4 = s4;
    }
};

// gpca_assoc_logistic_score (kCorrNone, corr = nullptr), gpca_assoc_logistic_spa and gpca_assoc_logistic_firth: one path; a correction
// only adds to it.  corr_z = spa_z or firth_z; corr = the correction's output, [rows][T][4] or [rows][T][kAfiWidth]
enum Correction { kCorrNone, kCorrSpa, kCorrFirth };
// gpca_assoc_logistic_set (section a16): the band is the list of the sets' rows instead of [row0, row1), and Phi follows the finish kernel
struct SetCall { int32_t n_sets; const int64_t *off, *rows; double* phi; };
int assoc_logistic(gpca_handle* h, const std::string& f, const double* Y, int32_t T, const double* C, int32_t Pc, const uint8_t* include,
                   double max_vif, Correction mode, double corr_z, int64_t row0, int64_t row1, double* stats, double* corr, double* ua,
                   double* rowinfo, const SetCall* sc = nullptr);
}  // namespace

extern "C" int gpca_logistic_null(const double* y, const double* C, int32_t Pc, const uint8_t* include, int64_t N, double* alpha,
                                  double* mu, int32_t* iters) {
    if (!y || N < 1 || Pc < 0 || (Pc > 0 && !C) || (!alpha && !mu)) return GPCA_ERR_BAD_ARG;
    LogitDesign D;
    std::string msg;
    int rc = logit_design(C, Pc, include, N, D, nullptr, msg);
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
    return assoc_logistic(h, "gpca_assoc_logistic_score", Y, T, C, Pc, include, max_vif, kCorrNone, INFINITY, row0, row1, stats, nullptr, ua, rowinfo);
}

extern "C" int gpca_assoc_logistic_spa(gpca_handle* h, const double* Y, int32_t T, const double* C, int32_t Pc, const uint8_t* include,
                                       double max_vif, double spa_z, int64_t row0, int64_t row1, double* stats, double* spa, double* ua,
                                       double* rowinfo) {
    if (!h) return GPCA_ERR_BAD_ARG;
    return assoc_logistic(h, "gpca_assoc_logistic_spa", Y, T, C, Pc, include, max_vif, kCorrSpa, spa_z, row0, row1, stats, spa, ua, rowinfo);
}

extern "C" int gpca_assoc_logistic_firth(gpca_handle* h, const double* Y, int32_t T, const double* C, int32_t Pc, const uint8_t* include,
                                         double max_vif, double firth_z, int64_t row0, int64_t row1, double* stats, double* firth, double* ua,
                                         double* rowinfo) {
    if (!h) return GPCA_ERR_BAD_ARG;
    return assoc_logistic(h, "gpca_assoc_logistic_firth", Y, T, C, Pc, include, max_vif, kCorrFirth, firth_z, row0, row1, stats, firth, ua, rowinfo);
}

extern "C" int gpca_assoc_logistic_set(gpca_handle* h, const double* Y, int32_t T, const double* C, int32_t Pc, const uint8_t* include,
                                       double max_vif, int32_t n_sets, const int64_t* set_off, const int64_t* set_rows, double* stats,
                                       double* ua, double* rowinfo, double* phi) {
    if (!h) return GPCA_ERR_BAD_ARG;
    const SetCall sc{n_sets, set_off, set_rows, phi};
    return assoc_logistic(h, "gpca_assoc_logistic_set", Y, T, C, Pc, include, max_vif, kCorrNone, INFINITY, 0, 0, stats, nullptr, ua, rowinfo, &sc);
}

namespace {
// the sets of a call, checked: the original row of every listed row and the strips of the lower triangles (plan_math.h: AsgStrip)
int set_plan(gpca_handle* h, const std::string& f, const SetCall& sc, int T, std::vector<int64_t>& lrows, std::vector<AsgStrip>& strips,
             int64_t& tri_total) {
    const int64_t K = h->n_pca;
    if (sc.n_sets < 1 || !sc.off || !sc.rows) return fail(h, GPCA_ERR_BAD_ARG, f + ": n_sets >= 1, set_off and set_rows are required");
    if (sc.off[0] != 0) return fail(h, GPCA_ERR_BAD_ARG, f + ": set_off[0] must be 0");
    tri_total = 0;
    for (int32_t s = 0; s < sc.n_sets; ++s) {
        const int64_t m = sc.off[s + 1] - sc.off[s];
        if (m < 1 || m > GPCA_SET_MAX_ROWS)
            return fail(h, GPCA_ERR_BAD_ARG, f + ": set " + std::to_string(s) + " lists " + std::to_string(m) + " rows: 1 to " +
                                                 std::to_string(GPCA_SET_MAX_ROWS) + " are allowed");
        for (int64_t i = sc.off[s]; i < sc.off[s + 1]; ++i) {
            const int64_t r = sc.rows[i];
            if (r < 0 || r >= K)
                return fail(h, GPCA_ERR_BAD_ARG, f + ": set " + std::to_string(s) + ": row " + std::to_string(r) + " is outside [0, K) (K = " +
                                                     std::to_string(K) + " kept rows)");
            if (i > sc.off[s] && r <= sc.rows[i - 1])
                return fail(h, GPCA_ERR_BAD_ARG, f + ": set " + std::to_string(s) + ": its rows are not strictly ascending");
            lrows.push_back(h->pca_rows[(size_t)r]);
        }
        for (int q = 0; q < asg_strips((int)m); ++q) strips.push_back(AsgStrip{sc.off[s], tri_total * (int64_t)T, (int32_t)m, (int32_t)q});
        tri_total += asg_tri(m);
    }
    return GPCA_OK;
}

int assoc_logistic(gpca_handle* h, const std::string& f, const double* Y, int32_t T, const double* C, int32_t Pc, const uint8_t* include,
                   double max_vif, Correction mode, double corr_z, int64_t row0, int64_t row1, double* stats, double* corr, double* ua,
                   double* rowinfo, const SetCall* sc) {
    LOCK(h);
    const bool with_spa = mode == kCorrSpa, with_firth = mode == kCorrFirth, with_corr = mode != kCorrNone;
    CHK(asc_check_call(h, f, T >= 1 && Pc >= 0 && (int64_t)T * ((int64_t)Pc + 3) <= kAsrMaxCols,
                       "T >= 1, Pc >= 0 and T (Pc + 3) <= " + std::to_string(kAsrMaxCols), Y, C, Pc,
                       with_corr ? (corr ? nullptr : (with_spa ? "spa is required" : "firth is required"))
                       : sc      ? (sc->phi ? nullptr : "phi is required")
                                 : (!stats && !ua && !rowinfo ? "stats, ua and rowinfo are all NULL" : nullptr),
                       row0, row1, max_vif,
                       with_spa && !spa_z_ok(corr_z)       ? "spa_z must be at least 0.5, or +inf for no correction"
                       : with_firth && !firth_z_ok(corr_z) ? "firth_z must be at least 0, or +inf for no correction"
                                                           : nullptr));
    const int64_t N = h->N;
    const int L = asr_cols(T, Pc), P = Pc + 1;
    const int64_t npad = asc_npad(N);
    // (a set call: the band of the kernels below is the list, rows [0, listed) of its own kept-row map)
    std::vector<int64_t> lrows;
    std::vector<AsgStrip> strips;
    int64_t tri_total = 0;
    if (sc) {
        CHK(set_plan(h, f, *sc, T, lrows, strips, tri_total));
        row0 = 0; row1 = (int64_t)lrows.size();
    }

    // host: the design, then per trait the null fit and its Pc + 3 columns
    LogitDesign D;
    std::string msg;
    std::vector<unsigned> incw;
    int rc = logit_design(C, Pc, include, N, D, &incw, msg);
    if (rc != GPCA_OK) return fail(h, rc, f + ": " + msg);
    const int64_t ns = (int64_t)D.S.size();
    std::vector<float> Bt((size_t)asc_b_capacity(N, L), 0.0f);
    // (a correction's: Z_t = X L_t^-T and mu_t in f64, 0 outside S and past N; with spa_z / firth_z = +inf no item is corrected: the flag
    // kernel alone runs, and the correction's inputs and workspace are neither built nor allocated)
    const bool correct = with_corr && std::isfinite(corr_z);
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
            asc_solve_lt(A, P, ns, D.X.data(), w.data(), col.data());            // A L^T = W X
            for (int64_t i = 0; i < ns; ++i) {
                const size_t n = (size_t)D.S[(size_t)i];
                Bt[(size_t)asr_col_w(t) * (size_t)npad + n] = (float)w[(size_t)i];
                Bt[(size_t)asr_col_r(T, t) * (size_t)npad + n] = (float)(Y[(int64_t)n * T + t] - mu[(size_t)i]);
                for (int j = 0; j < P; ++j) Bt[(size_t)asr_col_a(T, Pc, t, j) * (size_t)npad + n] = (float)col[(size_t)j * (size_t)ns + (size_t)i];
            }
            if (!correct) continue;
            asc_solve_lt(A, P, ns, D.X.data(), nullptr, zc.data());               // Z L^T = X
            for (int64_t i = 0; i < ns; ++i) {
                const size_t n = (size_t)D.S[(size_t)i];
                muh[(size_t)t * (size_t)gpad + n] = mu[(size_t)i];
                for (int j = 0; j < P; ++j) Zh[((size_t)t * P + (size_t)j) * (size_t)gpad + n] = zc[(size_t)j * (size_t)ns + (size_t)i];
            }
        }
    }
    const int64_t rows = row1 - row0;
    if (rows == 0) return GPCA_OK;
    const int64_t out_cap = with_firth ? afi_out_capacity(rows, T) : asp_out_capacity(rows, T);
    const bool dstats = stats || with_corr;                     // (the flag kernel reads z from the device's stats)
    if (asr_count_blocks(rows) >= ((int64_t)1 << 31)) return fail(h, GPCA_ERR_BAD_ARG, f + ": the band makes 2^31 or more workgroups: ask for fewer rows");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->st));
    CHK(preflight_device_memory(h, f.c_str(), sc ? "the sets need" : "the band needs",
                                (sc ? asg_call_bytes(N, rows, (int64_t)strips.size(), tri_total, T, Pc, dstats, ua != nullptr, rowinfo != nullptr)
                                    : asr_call_bytes(N, rows, T, Pc, dstats, ua != nullptr, rowinfo != nullptr, with_corr ? out_cap : 0, correct)) +
                                    (double)(64 << 20)));
    const bool packed = h->storage == GPCA_STORE_2BIT;
    const auto [G, ldr] = panel_rows(h, resident_view(h));
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
    if (sc) {
        HIPCHK(dalloc(ws.lrows, (size_t)asg_rows_capacity(rows))); HIPCHK(dalloc(ws.strips, (size_t)asg_strip_capacity((int64_t)strips.size())));
        HIPCHK(dalloc(ws.phi, (size_t)asg_phi_capacity(tri_total, T)));
        HIPCHK(hipMemcpyAsync(ws.lrows, lrows.data(), lrows.size() * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ws.strips, strips.data(), strips.size() * sizeof(AsgStrip), hipMemcpyHostToDevice, st));
    }
    const int64_t* krows = sc ? ws.lrows : h->d_pca_rows;
    if (with_corr) {
        HIPCHK(dalloc(ws.corr, (size_t)out_cap)); HIPCHK(dalloc(ws.list, (size_t)asp_list_capacity(rows, T)));
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
        if (launch_assoc_score_count(st, G, packed, ldr, krows, N, ws.incw, row0, row1, ws.sums, ws.bad) != 0)
            return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
        HIPCHK(hipGetLastError());
    }
    {
        // flops as for k_assoc, the d product over the padded columns plus the q product over its one block
        ScopedTimer t(h, "assoc_score", 2.0 * (double)rows * (double)N * (double)(asc_lpad(L) + 32), gbytes);
        if (launch_assoc_score(st, G, packed, ldr, krows, N, ws.Bt, ws.incw, T, L, row0, row1, ws.sums, ws.dv) != 0)
            return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
        HIPCHK(hipGetLastError());
    }
    launch_assoc_score_finish(st, ws.dv, ws.sums, T, Pc, max_vif, rows, ws.stats, ws.ua, ws.info);
    HIPCHK(hipGetLastError());
    if (with_corr) {
        ScopedTimer t(h, with_firth ? "assoc_firth" : "assoc_spa", 0.0, 0.0);
        const int64_t items = rows * (int64_t)T;
        int64_t forced = 0;
        if (const char* e = std::getenv("GPCA_ASP_SLOTS")) forced = std::strtoll(e, nullptr, 10);   // read per call: the tests' way to every walk edge
        const int64_t slots = asp_clamp_slots(N, forced);
        for (int64_t item0 = 0; item0 < items; item0 += kAspListItems) {
            HIPCHK(hipMemsetAsync(ws.count, 0, 4, st));
            const int64_t nitems = std::min<int64_t>(kAspListItems, items - item0);
            if (with_firth) launch_assoc_firth_flag(st, ws.stats, T, item0, nitems, corr_z, ws.corr, ws.list, ws.count);
            else launch_assoc_spa_flag(st, ws.stats, ws.dv, T, Pc, item0, nitems, corr_z, ws.corr, ws.list, ws.count);
            HIPCHK(hipGetLastError());
            if (!correct) continue;
            if ((with_firth ? launch_assoc_firth : launch_assoc_spa)(st, G, packed, ldr, krows, N, ws.incw, ws.sums, ws.dv, ws.Z, ws.mu, T, Pc,
                                                                     row0, item0, ws.list, ws.count, ws.g, ws.corr, slots) != 0)
                return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
            HIPCHK(hipGetLastError());
        }
    }
    if (sc) {
        // flops: the XX product over the tiles of the strips (the M products run only where calls are missing)
        ScopedTimer t(h, "assoc_set_gram", 2.0 * (double)tri_total * (double)T * (double)N, gbytes * (double)T);
        if (launch_assoc_set_gram(st, G, packed, ldr, ws.lrows, N, ws.Bt, ws.incw, T, ws.sums, ws.strips, (int64_t)strips.size(), ws.phi) != 0 ||
            launch_assoc_set_finish(st, ws.dv, ws.sums, T, Pc, ws.strips, (int64_t)strips.size(), ws.phi) != 0)
            return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
        HIPCHK(hipGetLastError());
    }
    CHK(asc_check_genotypes(h, f, ws.bad, st));
    return asc_copy_outputs(h, st, {{sc ? sc->phi : nullptr, ws.phi, sc ? asg_phi_capacity(tri_total, T) : 0}, {stats, ws.stats, asr_stats_capacity(rows, T)}, {ua, ws.ua, asr_ua_capacity(rows, T, Pc)},
                                    {rowinfo, ws.info, asr_info_capacity(rows)}, {corr, ws.corr, with_corr ? out_cap : 0}});
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

extern "C" int gpca_firth_log10p(const double* gt, const double* mu, int64_t n, double u, double* out) {
#pragma clang fp contract(off)
    if (!gt || !mu || n < 1 || !out || !std::isfinite(u)) return GPCA_ERR_BAD_ARG;
    double V = 0.0, gmax = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        if (!std::isfinite(gt[i]) || !(mu[i] >= 0.0 && mu[i] <= 1.0)) return GPCA_ERR_BAD_ARG;
        gmax = std::fmax(gmax, std::fabs(gt[i]));
        V = V + (1.0 - mu[i]) * mu[i] * (gt[i] * gt[i]);
    }
    const HostFirthEval ev{gt, mu, n};
    FirthResult r;
    firth_item(ev, u, gmax, u == 0.0 ? 0.0 : spa_normal_log10p(u / std::sqrt(V)), r);
    out[0] = r.log10p; out[1] = (double)r.status; out[2] = r.beta; out[3] = r.se; out[4] = r.lrt;
    return GPCA_OK;
}

// gpca_set_test (section a16): the burden and SKAT rules of one set, host only
namespace {
constexpr int kSetMaxSteps = 200;
constexpr double kSetStop = 1e-10, kSetMinZ = 0.5, kSetKeep = 1e5;
// -log10 P(Q > q) by Satterthwaite's scaled chi^2 and the Wilson-Hilferty cube root
double set_bulk(double Q, double c1, double c2) {
#pragma clang fp contract(off)
    const double kappa = c2 / c1, nu = c1 * c1 / c2, v = 2.0 / (9.0 * nu);
    const double x = (std::cbrt(Q / (kappa * nu)) - (1.0 - v)) / std::sqrt(v);
    return spa_upper_log10p(x);
}
}  // namespace

extern "C" int gpca_set_test(const double* u, const double* phi, const double* weight, int32_t m, double* out) {
#pragma clang fp contract(off)
    if (!u || !phi || !out || m < 1 || m > GPCA_SET_MAX_ROWS) return GPCA_ERR_BAD_ARG;
    if (weight)
        for (int i = 0; i < m; ++i) if (std::isnan(weight[i]) || weight[i] < 0.0) return GPCA_ERR_BAD_ARG;
    auto P = [&](int i, int j) { return i >= j ? phi[(size_t)i * ((size_t)i + 1) / 2 + (size_t)j] : phi[(size_t)j * ((size_t)j + 1) / 2 + (size_t)i]; };
    std::vector<int> used;
    std::vector<double> om;
    for (int i = 0; i < m; ++i) {
        const double w = weight ? weight[i] : 1.0, d = P(i, i);
        if (std::isfinite(u[i]) && std::isfinite(d) && d > 0.0 && std::isfinite(w) && w > 0.0) { used.push_back(i); om.push_back(w); }
    }
    const int n = (int)used.size();
    const double nan = std::nan("");
    out[0] = (double)n;
    for (int k = 1; k < 10; ++k) out[k] = nan;
    out[7] = 0.0;
    if (n == 0) return GPCA_OK;
    // A = diag(omega) Phi diag(omega) over the used rows
    std::vector<double> A((size_t)n * (size_t)n), lam((size_t)n), vec((size_t)n * (size_t)n);
    bool finite = true;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const double a = (om[(size_t)i] * P(used[(size_t)i], used[(size_t)j])) * om[(size_t)j];
            A[(size_t)i * n + j] = a;
            finite = finite && std::isfinite(a);
        }
    double B = 0.0, v = 0.0, Q = 0.0;
    for (int i = 0; i < n; ++i) {
        const double t = om[(size_t)i] * u[used[(size_t)i]];
        B = B + t;
        Q = Q + t * t;
        for (int j = 0; j < n; ++j) v = v + A[(size_t)i * n + j];
    }
    if (v > 0.0) {
        const double rt = std::sqrt(v);
        out[1] = B / v; out[2] = 1.0 / rt; out[3] = B / rt; out[4] = spa_normal_log10p(B / rt);
    }
    out[5] = Q;
    if (!finite || gpca_host_eigh_desc(A.data(), n, lam.data(), vec.data()) != GPCA_OK) return GPCA_OK;
    double pos = 0.0;
    int npos = 0;
    for (int i = 0; i < n; ++i) if (lam[(size_t)i] >= 0.0) { pos = pos + lam[(size_t)i]; ++npos; }
    const double keep = npos ? pos / (double)npos / kSetKeep : 0.0;
    int nl = 0;
    while (nl < n && lam[(size_t)nl] > keep) ++nl;                       // (descending: the kept ones lead)
    double c1 = 0.0, c2 = 0.0;
    for (int i = 0; i < nl; ++i) { c1 = c1 + lam[(size_t)i]; c2 = c2 + lam[(size_t)i] * lam[(size_t)i]; }
    if (nl == 0) return GPCA_OK;
    const double zq = (Q - c1) / std::sqrt(2.0 * c2);
    out[8] = zq;
    const double bulk = set_bulk(Q, c1, c2);
    out[6] = bulk;
    if (!(zq >= kSetMinZ)) return GPCA_OK;
    // Kuonen's saddle point: the root of K'(zeta) = Q on (0, 1 / (2 lambda_1)) by a bracketed Newton
    const double ub = 1.0 / (2.0 * lam[0]);
    double lo = 0.0, hi = ub, zeta = (Q - c1) / (2.0 * c2);
    if (!(zeta > lo && zeta < hi)) zeta = 0.5 * (lo + hi);
    auto k12 = [&](double z, double& k1, double& k2) {
        double s1 = 0.0, s2 = 0.0;
        for (int i = 0; i < nl; ++i) {
            const double l = lam[(size_t)i], d = 1.0 - 2.0 * z * l, r = l / d;
            s1 = s1 + r; s2 = s2 + r * r;
        }
        k1 = s1; k2 = 2.0 * s2;
    };
    bool found = false;
    for (int rep = 0; rep < kSetMaxSteps && !found; ++rep) {
        double k1, k2;
        k12(zeta, k1, k2);
        const double f = k1 - Q;
        if (!std::isfinite(f)) break;
        if (f > 0.0) hi = zeta; else lo = zeta;
        double zn = zeta - f / k2;
        if (!(zn > lo && zn < hi)) zn = 0.5 * (lo + hi);
        found = std::fabs(zn - zeta) <= kSetStop * ub;
        zeta = zn;
    }
    out[9] = zeta;
    out[7] = 2.0;
    if (!found) return GPCA_OK;
    double K = 0.0, k1, k2;
    for (int i = 0; i < nl; ++i) K = K + std::log1p(-2.0 * zeta * lam[(size_t)i]);
    K = -0.5 * K;
    k12(zeta, k1, k2);
    const double w = std::sqrt(2.0 * (zeta * Q - K)), vv = zeta * std::sqrt(k2);
    const double r = w + std::log(vv / w) / w;
    if (!std::isfinite(r) || !(r > 0.0)) return GPCA_OK;
    out[6] = spa_upper_log10p(r);
    out[7] = 1.0;
    return GPCA_OK;
}

// (spa_math.h holds the function: the kernels of assoc_spa.hip use it too)
extern "C" double gpca_normal_log10p(double z) { return spa_normal_log10p(z); }
