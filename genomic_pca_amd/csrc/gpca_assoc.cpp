// gpca_assoc_linear / gpca_student_t_log10p (include/gpca.h section a12): the linear association scan.  The traits and covariates
// are reduced on the host in f64 to B = [Y~ | Q] (Q by Cholesky of the centred, unit-scaled covariates: at most 63 x 63); one pass
// over the band's kept rows multiplies them on the matrix cores (k_assoc), a second kernel makes the statistics (k_assoc_finish).
// The call has its own workspace, allocated and freed per call, and reads nothing of the handle's state but the genotypes and the
// list of kept rows.
// The host front end that this scan shares with the logistic scans of gpca_assoc_score.cpp is defined here too (declared in
// gpca_internal.h): the argument checks, S and the include words, the standardised covariates, the Cholesky factor, X L^-T, the
// invalid-genotype read-back and the copies of the outputs.
#include "gpca_internal.h"

using namespace gpca;

// ---- the host front end shared with gpca_assoc_score.cpp (declared in gpca_internal.h) ---------------------------------------
int asc_check_call(gpca_handle* h, const std::string& f, bool cols_ok, const std::string& cols_rule, const double* Y, const double* C, int Pc,
                   const char* out_err, int64_t row0, int64_t row1, double max_vif, const char* late_err) {
    if (!have_genotypes(h)) return fail(h, GPCA_ERR_STATE, f + ": no genotypes resident");
    if (h->sm.on)
        return fail(h, GPCA_ERR_STATE, f + ": the handle streams its matrix in panels, which is not implemented");
    if (multi_rank(h)) return fail(h, GPCA_ERR_STATE, f + ": the handle holds a shard of the rows, which is not implemented");
    if (!h->have_stats) return fail(h, GPCA_ERR_STATE, f + ": no standardisation: run gpca_snp_stats or gpca_set_standardization first");
    if (h->n_pca == 0) return fail(h, GPCA_ERR_STATE, f + ": no kept row (the keep mask is empty)");
    const int64_t K = h->n_pca;
    if (!cols_ok) return fail(h, GPCA_ERR_BAD_ARG, f + ": " + cols_rule + " are required");
    if (!Y) return fail(h, GPCA_ERR_BAD_ARG, f + ": Y is required");
    if (Pc > 0 && !C) return fail(h, GPCA_ERR_BAD_ARG, f + ": C is required when Pc > 0");
    if (out_err) return fail(h, GPCA_ERR_BAD_ARG, f + ": " + out_err);
    if (row0 < 0 || row1 < row0 || row1 > K)
        return fail(h, GPCA_ERR_BAD_ARG, f + ": rows must satisfy 0 <= row0 <= row1 <= K (K = " + std::to_string(K) + " kept rows)");
    if (!(max_vif >= 1.0) || !std::isfinite(max_vif)) return fail(h, GPCA_ERR_BAD_ARG, f + ": max_vif must be finite and at least 1");
    if (late_err) return fail(h, GPCA_ERR_BAD_ARG, f + ": " + late_err);
    if (h->N >= ((int64_t)1 << 30)) return fail(h, GPCA_ERR_BAD_ARG, f + ": 2^30 or more samples (the per-row sums are 32-bit)");
    return GPCA_OK;
}

void asc_sample_set(const uint8_t* include, int64_t N, std::vector<int64_t>& S, std::vector<unsigned>* incw) {
    S.clear();
    S.reserve((size_t)N);
    for (int64_t n = 0; n < N; ++n) if (!include || include[n]) S.push_back(n);
    if (!incw) return;
    incw->assign((size_t)asc_inc_capacity(N), 0u);
    for (int64_t n : S) (*incw)[(size_t)(n >> 5)] |= 1u << (int)(n & 31);
}

int asc_standardise(const double* C, int Pc, const std::vector<int64_t>& S, double* X, std::string& msg) {
    const int64_t ns = (int64_t)S.size();
    for (int j = 0; j < Pc; ++j) {
        double* c = X + (size_t)j * (size_t)ns;
        double sum = 0.0, raw = 0.0, ss = 0.0;
        for (int64_t i = 0; i < ns; ++i) {
            c[i] = C[S[(size_t)i] * Pc + j];
            if (!std::isfinite(c[i])) { msg = "C[" + std::to_string(S[(size_t)i]) + "][" + std::to_string(j) + "] is not finite"; return GPCA_ERR_BAD_ARG; }
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

int asc_cholesky(const double* X, int P, int64_t ns, const double* w, bool (*accept)(double d, double diag), std::vector<double>& A,
                 std::string& msg) {
    A.assign((size_t)P * P, 0.0);
    for (int i = 0; i < P; ++i)
        for (int j = 0; j <= i; ++j) {
            const double *a = X + (size_t)i * (size_t)ns, *b = X + (size_t)j * (size_t)ns;
            double s = 0.0;
            if (w) for (int64_t n = 0; n < ns; ++n) s += w[n] * a[n] * b[n];
            else for (int64_t n = 0; n < ns; ++n) s += a[n] * b[n];
            A[(size_t)i * P + j] = s;
        }
    for (int j = 0; j < P; ++j) {
        const double diag = A[(size_t)j * P + j];
        double d = diag;
        for (int k = 0; k < j; ++k) d -= A[(size_t)j * P + k] * A[(size_t)j * P + k];
        if (!accept(d, diag)) {
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

void asc_solve_lt(const std::vector<double>& A, int P, int64_t ns, const double* X, const double* w, double* out) {
    for (int j = 0; j < P; ++j) {
        double* a = out + (size_t)j * (size_t)ns;
        const double* x = X + (size_t)j * (size_t)ns;
        if (w) for (int64_t i = 0; i < ns; ++i) a[i] = w[i] * x[i];
        else if (a != x) for (int64_t i = 0; i < ns; ++i) a[i] = x[i];
        for (int k = 0; k < j; ++k) {
            const double l = A[(size_t)j * P + k];
            const double* ak = out + (size_t)k * (size_t)ns;
            for (int64_t i = 0; i < ns; ++i) a[i] -= l * ak[i];
        }
        const double inv = 1.0 / A[(size_t)j * P + j];
        for (int64_t i = 0; i < ns; ++i) a[i] *= inv;
    }
}

int asc_check_genotypes(gpca_handle* h, const std::string& f, const unsigned long long* d_bad, hipStream_t st) {
    unsigned long long bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (bad != ~0ull)
        return fail(h, GPCA_ERR_INVALID_GENOTYPE, f + ": row " + std::to_string(bad) + " holds a genotype outside {0, 1, 2, missing}");
    return GPCA_OK;
}

int asc_copy_outputs(gpca_handle* h, hipStream_t st, std::initializer_list<AscOutput> outs) {
    for (const AscOutput& o : outs)
        if (o.host) HIPCHK(hipMemcpyAsync(o.host, o.dev, (size_t)o.elems * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GPCA_OK;
}

namespace {
struct AscWs {
    float* Bt = nullptr;
    unsigned *incw = nullptr, *sums = nullptr;
    double *xb = nullptr, *yy = nullptr, *stats = nullptr, *info = nullptr;
    unsigned long long* bad = nullptr;
    ~AscWs() { dfree(Bt); dfree(incw); dfree(sums); dfree(xb); dfree(yy); dfree(stats); dfree(info); dfree(bad); }
};

}  // namespace

// Host step: S = the included samples; Q = an orthonormal basis of the columns of C centred over S (each scaled to unit norm, then
// Q = C L^-T with C^T C = L L^T); Y~ = Y centred over S minus Q Q^T Y (taken out twice, so that what rounding leaves of the first pass
// goes too); yy [T] = |Y~_t|^2; incw = the mask as bits.  A trait column is treated on its own: its Y~ and yy do not depend on T.
int asc_design_host(gpca_handle* h, const std::string& f, const double* Y, int64_t T, const double* C, int Pc, const uint8_t* include,
                    AscDesign& d, std::vector<unsigned>& incw, std::vector<double>& yy) {
    const int64_t N = h->N;
    std::vector<int64_t>& S = d.S;
    asc_sample_set(include, N, S, &incw);
    const int64_t ns = (int64_t)S.size();
    if (ns - Pc - 2 < 1)
        return fail(h, GPCA_ERR_BAD_ARG, f + ": " + std::to_string(ns) + " included samples leave df = n - Pc - 2 < 1");
    // (sample-major: the first entry that is not finite in the order of the caller's rows, ahead of the column-major standardisation)
    for (int64_t n : S) {
        for (int64_t t = 0; t < T; ++t)
            if (!std::isfinite(Y[n * T + t])) return fail(h, GPCA_ERR_BAD_ARG, f + ": Y[" + std::to_string(n) + "][" + std::to_string(t) + "] is not finite");
        for (int j = 0; j < Pc; ++j)
            if (!std::isfinite(C[n * Pc + j])) return fail(h, GPCA_ERR_BAD_ARG, f + ": C[" + std::to_string(n) + "][" + std::to_string(j) + "] is not finite");
    }
    // the covariates over S, column-major, centred and scaled to unit norm; A = Cc^T Cc = L L^T (unit diagonal: a pivot that falls to
    // 1e-10 means the columns are collinear to working precision); Q L^T = Cc, in place
    std::vector<double>& Cc = d.Q;
    std::vector<double>& Yc = d.Yc;
    Cc.assign((size_t)Pc * (size_t)ns, 0.0); Yc.assign((size_t)T * (size_t)ns, 0.0);
    std::vector<double> A;
    std::string msg;
    int rc = asc_standardise(C, Pc, S, Cc.data(), msg);
    if (rc == GPCA_OK) rc = asc_cholesky(Cc.data(), Pc, ns, nullptr, [](double d, double) { return d > 1e-10; }, A, msg);
    if (rc != GPCA_OK) return fail(h, rc, f + ": " + msg);
    asc_solve_lt(A, Pc, ns, Cc.data(), nullptr, Cc.data());
    yy.assign((size_t)T, 0.0);
    // one trait: false when it is constant once the covariates are taken out.  It reads and writes its own column only, so the traits
    // of a wide call may go to several threads without moving a bit.
    auto one = [&](int64_t t) {
        double* y = &Yc[(size_t)t * (size_t)ns];
        double sum = 0.0;
        for (int64_t i = 0; i < ns; ++i) { y[i] = Y[S[(size_t)i] * T + t]; sum += y[i]; }
        const double mean = sum / (double)ns;
        for (int64_t i = 0; i < ns; ++i) y[i] -= mean;
        for (int pass = 0; pass < 2; ++pass)
            for (int j = 0; j < Pc; ++j) {
                const double* q = &Cc[(size_t)j * (size_t)ns];
                double dot = 0.0;
                for (int64_t i = 0; i < ns; ++i) dot += q[i] * y[i];
                for (int64_t i = 0; i < ns; ++i) y[i] -= dot * q[i];
            }
        double ss = 0.0;
        for (int64_t i = 0; i < ns; ++i) ss += y[i] * y[i];
        if (!(ss > 0.0) || !std::isfinite(ss)) return false;
        yy[(size_t)t] = ss;
        return true;
    };
    // (gpca_assoc_linear's at most 64 traits stay on the caller's thread; GPCA_DESIGN_THREADS, default 8, for kAscDesignPerThread
    // traits per thread and more)
    constexpr int64_t kAscDesignPerThread = 128;
    int want = 8;
    if (const char* e = std::getenv("GPCA_DESIGN_THREADS")) want = std::atoi(e);
    const int64_t nthr = std::max<int64_t>(1, std::min<int64_t>({(int64_t)want, 64, (int64_t)std::max(1u, std::thread::hardware_concurrency()), T / kAscDesignPerThread}));
    std::atomic<int64_t> bad(T);                                                      // the first trait that fails
    auto walk = [&](int64_t k) {
        for (int64_t t = k; t < T && t < bad.load(std::memory_order_relaxed); t += nthr)
            if (!one(t)) {
                int64_t cur = bad.load();
                while (t < cur && !bad.compare_exchange_weak(cur, t)) {}
            }
    };
    if (nthr == 1) walk(0);
    else {
        std::vector<std::thread> th;
        for (int64_t k = 0; k < nthr; ++k) th.emplace_back(walk, k);
        for (std::thread& x : th) x.join();
    }
    if (bad.load() < T)
        return fail(h, GPCA_ERR_BAD_ARG, f + ": trait " + std::to_string(bad.load()) + " is constant over the included samples once the covariates are taken out (yy = 0)");
    return GPCA_OK;
}

void asc_design_rows(const AscDesign& d, const std::vector<double>& cols, int64_t ncols, int64_t npad, float* Bt) {
    const int64_t ns = (int64_t)d.S.size();
    for (int64_t t = 0; t < ncols; ++t) {
        const double* y = &cols[(size_t)t * (size_t)ns];
        float* o = Bt + (size_t)t * (size_t)npad;
        for (int64_t i = 0; i < ns; ++i) o[(size_t)d.S[(size_t)i]] = (float)y[i];
    }
}

namespace {
// gpca_assoc_linear's panel: Bt [lpad][npad] = (float)[Y~ | Q]^T, zero outside S
int asc_design(gpca_handle* h, const double* Y, int T, const double* C, int Pc, const uint8_t* include, std::vector<float>& Bt,
               std::vector<unsigned>& incw, std::vector<double>& yy, int64_t& n_inc) {
    static const std::string f("gpca_assoc_linear");
    const int64_t N = h->N, npad = asc_npad(N);
    AscDesign d;
    CHK(asc_design_host(h, f, Y, T, C, Pc, include, d, incw, yy));
    n_inc = (int64_t)d.S.size();
    Bt.assign((size_t)asc_b_capacity(N, T + Pc), 0.0f);
    asc_design_rows(d, d.Yc, T, npad, Bt.data());
    asc_design_rows(d, d.Q, Pc, npad, Bt.data() + (size_t)T * (size_t)npad);
    return GPCA_OK;
}
}  // namespace

extern "C" int gpca_assoc_linear(gpca_handle* h, const double* Y, int32_t T, const double* C, int32_t Pc, const uint8_t* include,
                                 double max_vif, int64_t row0, int64_t row1, double* stats, double* xb, double* rowinfo) {
    if (!h) return GPCA_ERR_BAD_ARG;
    LOCK(h);
    static const std::string f("gpca_assoc_linear");
    CHK(asc_check_call(h, f, T >= 1 && Pc >= 0 && (int64_t)T + Pc <= kAscMaxCols, "T >= 1, Pc >= 0 and T + Pc <= " + std::to_string(kAscMaxCols), Y,
                       C, Pc, !stats && !xb && !rowinfo ? "stats, xb and rowinfo are all NULL" : nullptr, row0, row1, max_vif));
    const int64_t N = h->N;
    const int L = T + Pc;
    std::vector<float> Bt; std::vector<unsigned> incw; std::vector<double> yy;
    int64_t n_inc = 0;
    CHK(asc_design(h, Y, T, C, Pc, include, Bt, incw, yy, n_inc));
    const int64_t rows = row1 - row0;
    if (rows == 0) return GPCA_OK;
    if (asc_row_blocks(rows) >= ((int64_t)1 << 31)) return fail(h, GPCA_ERR_BAD_ARG, f + ": the band makes 2^31 or more workgroups: ask for fewer rows");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->st));
    CHK(preflight_device_memory(h, f.c_str(), "the band needs",
                                4.0 * (double)asc_b_capacity(N, L) + 4.0 * (double)asc_inc_capacity(N) + 8.0 * (double)asc_xb_capacity(rows, L) +
                                    4.0 * (double)asc_sums_capacity(rows) + (stats ? 8.0 * (double)asc_stats_capacity(rows, T) : 0.0) +
                                    (rowinfo ? 8.0 * (double)asc_info_capacity(rows) : 0.0) + 8.0 * T + (double)(64 << 20)));
    const bool packed = h->storage == GPCA_STORE_2BIT;
    const auto [G, ldr] = panel_rows(h, resident_view(h));
    hipStream_t st = h->st;
    AscWs ws;
    HIPCHK(dalloc(ws.Bt, Bt.size())); HIPCHK(dalloc(ws.incw, incw.size())); HIPCHK(dalloc(ws.yy, (size_t)T)); HIPCHK(dalloc(ws.bad, 1));
    HIPCHK(dalloc(ws.xb, (size_t)asc_xb_capacity(rows, L))); HIPCHK(dalloc(ws.sums, (size_t)asc_sums_capacity(rows)));
    if (stats) HIPCHK(dalloc(ws.stats, (size_t)asc_stats_capacity(rows, T)));
    if (rowinfo) HIPCHK(dalloc(ws.info, (size_t)asc_info_capacity(rows)));
    HIPCHK(hipMemcpyAsync(ws.Bt, Bt.data(), Bt.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ws.incw, incw.data(), incw.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ws.yy, yy.data(), (size_t)T * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(ws.bad, 0xff, 8, st));
    {
        // flops as the bench and DESIGN count them: the d product over the padded columns (the e product runs only where calls are missing)
        ScopedTimer t(h, "assoc", 2.0 * (double)rows * (double)N * (double)asc_lpad(L), (double)rows * (double)N * (packed ? 0.25 : 1.0));
        if (launch_assoc(st, G, packed, ldr, h->d_pca_rows, N, ws.Bt, ws.incw, L, row0, row1, ws.xb, ws.sums, ws.bad) != 0)
            return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
        HIPCHK(hipGetLastError());
    }
    if (stats || rowinfo) {
        launch_assoc_finish(st, ws.xb, ws.sums, ws.yy, T, L, (double)(n_inc - Pc - 2), max_vif, rows, ws.stats, ws.info);
        HIPCHK(hipGetLastError());
    }
    CHK(asc_check_genotypes(h, f, ws.bad, st));
    return asc_copy_outputs(h, st, {{stats, ws.stats, asc_stats_capacity(rows, T)}, {xb, ws.xb, asc_xb_capacity(rows, L)},
                                    {rowinfo, ws.info, asc_info_capacity(rows)}});
}

namespace {
// ln Gamma(a + 1/2) - ln Gamma(a): Stirling's series of the difference for a >= 10 (its first omitted term is below 1e-12 there, and
// nothing large is subtracted), lgamma below
double lgamma_half_step(double a) {
    if (a < 10.0) return std::lgamma(a + 0.5) - std::lgamma(a);
    auto tail = [](double z) {
        const double r = 1.0 / z, r2 = r * r;
        return r * (1.0 / 12.0 - r2 * (1.0 / 360.0 - r2 * (1.0 / 1260.0 - r2 * (1.0 / 1680.0))));
    };
    return (a * std::log1p(0.5 / a) - 0.5) + 0.5 * std::log(a) + (tail(a + 0.5) - tail(a));
}
// the continued fraction of the incomplete beta function (modified Lentz); converges quickly for x < (a + 1) / (a + b + 2)
double beta_cf(double a, double b, double x) {
    const double tiny = 1e-300, qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (std::fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double hh = d;
    for (int m = 1; m <= 200000; ++m) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d; if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d; hh *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d; if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        hh *= del;
        if (std::fabs(del - 1.0) < 1e-16) break;
    }
    return hh;
}
}  // namespace

// p = I_x(df / 2, 1 / 2), x = df / (df + t^2).  In the tail (x small) the logarithm of the prefactor and of the continued fraction
// are added, so nothing underflows; near t = 0 the complement 1 - I_{1 - x}(1 / 2, df / 2) goes through log1p.
extern "C" double gpca_student_t_log10p(double t, double df) {
    if (std::isnan(t) || !(df > 0.0) || !std::isfinite(df)) return std::nan("");
    if (std::isinf(t)) return INFINITY;
    if (t == 0.0) return 0.0;
    const double t2 = t * t, a = 0.5 * df, b = 0.5;
    const double x = df / (df + t2), ln_x = -std::log1p(t2 / df), ln_1mx = -std::log1p(df / t2);
    const double ln_beta = 0.5 * std::log(M_PI) - lgamma_half_step(a);      // ln B(a, 1/2)
    const double ln10 = std::log(10.0);
    if (x < (a + 1.0) / (a + b + 2.0)) {
        const double ln_p = a * ln_x + b * ln_1mx - std::log(a) - ln_beta + std::log(beta_cf(a, b, x));
        return -ln_p / ln10;
    }
    const double y = t2 / (df + t2);
    const double ln_q = b * ln_1mx + a * ln_x - std::log(b) - ln_beta + std::log(beta_cf(b, a, y));
    return -std::log1p(-std::exp(ln_q)) / ln10;
}
