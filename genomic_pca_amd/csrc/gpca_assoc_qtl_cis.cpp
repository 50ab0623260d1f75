// gpca_assoc_qtl_cis / gpca_qtl_perm_panel / gpca_qtl_perm_table / gpca_qtl_beta_approx (include/gpca.h section a25): cis-QTL mapping.
// The host step (asc_design_host on the G columns) and the per-row pass over the union of the windows (launch_assoc on the covariate
// basis, launch_assoc_finish) run once per call, exactly as gpca_assoc_qtl runs them.  The permutation table, Q, the residuals of all traits
// and S stay on the device for the call; per trait, k_qtl_perm_panel builds the panel of P + 1 columns, k_assoc_qtl_cis scans the window in
// launches of qtl_chunk_blocks(P + 1) row blocks and k_assoc_qtl_cis_best folds them (assoc_qtl_cis.hip).  The results come back once, after
// the last trait.  n_var is counted on the host from the per-row pass with the kernel's liveness rule.  The call has its own workspace,
// allocated and freed per call.  The table and the beta approximation are host rules.
#include "gpca_internal.h"
#include "philox.hpp"

#include <numeric>

using namespace gpca;

#pragma clang fp contract(off)

namespace {
struct CisWs {
    float *Bt = nullptr, *Qt = nullptr;
    unsigned *incw = nullptr, *sums = nullptr;
    uint32_t* perm = nullptr;
    int* S = nullptr;
    double *Q = nullptr, *resid = nullptr, *xbq = nullptr, *info = nullptr, *ws_r2 = nullptr, *ws_xb = nullptr, *run_r2 = nullptr, *run_xb = nullptr,
           *perm_r2 = nullptr, *best = nullptr;
    long long *ws_row = nullptr, *run_row = nullptr;
    unsigned long long* bad = nullptr;
    ~CisWs() {
        dfree(Bt); dfree(Qt); dfree(incw); dfree(sums); dfree(perm); dfree(S); dfree(Q); dfree(resid); dfree(xbq); dfree(info); dfree(ws_r2);
        dfree(ws_xb); dfree(run_r2); dfree(run_xb); dfree(perm_r2); dfree(best); dfree(ws_row); dfree(run_row); dfree(bad);
    }
};

// the first row of perm [P][n] that is not a permutation of 0 .. n - 1 (-1: none)
int64_t first_bad_perm_row(const uint32_t* perm, int64_t P, int64_t n) {
    std::vector<int64_t> seen((size_t)n, -1);
    for (int64_t p = 0; p < P; ++p)
        for (int64_t i = 0; i < n; ++i) {
            const uint32_t v = perm[p * n + i];
            if ((int64_t)v >= n || seen[(size_t)v] == p) return p;
            seen[(size_t)v] = p;
        }
    return -1;
}
}  // namespace

extern "C" int gpca_assoc_qtl_cis(gpca_handle* h, const double* Y, int64_t G, const double* C, int32_t Pc, const uint8_t* include, double max_vif,
                                  const int64_t* win, const uint32_t* perm, int32_t P, int64_t* n_var, int64_t* best_row, double* best_r2,
                                  double* best_stat, double* perm_r2) {
    if (!h) return GPCA_ERR_BAD_ARG;
    LOCK(h);
    static const std::string f("gpca_assoc_qtl_cis");
    const char* out_err = !win ? "win is required" : !n_var || !best_row || !best_r2 || !best_stat ? "n_var, best_row, best_r2 and best_stat are required"
                          : nullptr;
    const char* late_err = P < 0 || P > kQtlCisMaxPerm ? "P must lie in [0, 65535]" : P > 0 && !perm ? "perm is required when P > 0"
                           : P > 0 && !perm_r2 ? "perm_r2 is required when P > 0" : nullptr;
    CHK(asc_check_call(h, f, G >= 1 && G <= kQtlMaxTraits && Pc >= 0 && Pc <= kQtlMaxPc,
                       "1 <= G <= " + std::to_string(kQtlMaxTraits) + " and 0 <= Pc <= " + std::to_string(kQtlMaxPc), Y, C, Pc, out_err, 0, 0, max_vif,
                       late_err));
    const int64_t N = h->N, npad = asc_npad(N), K = h->n_pca;
    int64_t ulo = K, uhi = 0, wrows = 0;
    for (int64_t g = 0; g < G; ++g) {
        const int64_t lo = win[2 * g], hi = win[2 * g + 1];
        if (lo < 0 || hi < lo || hi > K)
            return fail(h, GPCA_ERR_BAD_ARG, f + ": the window of trait " + std::to_string(g) + " must satisfy 0 <= lo <= hi <= K (K = " +
                                                 std::to_string(K) + " kept rows)");
        if (hi > lo) { ulo = std::min(ulo, lo); uhi = std::max(uhi, hi); wrows = std::max(wrows, hi - lo); }
    }
    AscDesign d;
    std::vector<unsigned> incw; std::vector<double> yy;
    CHK(asc_design_host(h, f, Y, G, C, Pc, include, d, incw, yy));
    const int64_t n = (int64_t)d.S.size();
    if (P > 0) {
        const int64_t badrow = first_bad_perm_row(perm, P, n);
        if (badrow >= 0)
            return fail(h, GPCA_ERR_BAD_ARG, f + ": row " + std::to_string(badrow) + " of perm is not a permutation of 0 .. n - 1 (n = " +
                                                 std::to_string(n) + " included samples)");
    }
    const double nan = std::nan("");
    for (int64_t g = 0; g < G; ++g) {
        n_var[g] = 0; best_row[g] = -1; best_r2[g] = nan;
        best_stat[3 * g] = best_stat[3 * g + 1] = best_stat[3 * g + 2] = nan;
    }
    if (P > 0) std::fill(perm_r2, perm_r2 + G * (int64_t)P, nan);
    if (uhi <= ulo) return GPCA_OK;
    const int64_t rows = uhi - ulo, T = (int64_t)P + 1;
    if (asc_row_blocks(rows) >= ((int64_t)1 << 31)) return fail(h, GPCA_ERR_BAD_ARG, f + ": the windows span 2^31 or more workgroups: ask for fewer rows");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->st));
    CHK(preflight_device_memory(h, f.c_str(), "the windows need", qtl_cis_call_bytes(N, n, rows, wrows, G, P, Pc) + (double)(64 << 20)));
    int64_t forced = 0;
    if (const char* e = std::getenv("GPCA_QTL_TW")) {                                 // read per call: the tests' way to every strip edge
        forced = std::strtoll(e, nullptr, 10);
        if (forced < 1) forced = 1;
    }
    const int64_t chunk_blocks = qtl_chunk_blocks(T);
    const int Lq = qtl_cov_cols(Pc);

    std::vector<float> Qt((size_t)qtl_q_capacity(N, Pc), 0.0f);
    asc_design_rows(d, d.Q, Pc, npad, Qt.data());
    std::vector<int> S32((size_t)n);
    for (int64_t i = 0; i < n; ++i) S32[(size_t)i] = (int)d.S[(size_t)i];

    const bool packed = h->storage == GPCA_STORE_2BIT;
    const auto [Gm, ldr] = panel_rows(h, resident_view(h));
    hipStream_t st = h->st;
    CisWs ws;
    HIPCHK(dalloc(ws.Bt, (size_t)qtl_cis_panel_capacity(N, P))); HIPCHK(dalloc(ws.Qt, Qt.size())); HIPCHK(dalloc(ws.incw, incw.size()));
    HIPCHK(dalloc(ws.perm, (size_t)qtl_cis_table_capacity(P, n))); HIPCHK(dalloc(ws.S, (size_t)n)); HIPCHK(dalloc(ws.Q, (size_t)qtl_cis_q_capacity(Pc, n)));
    HIPCHK(dalloc(ws.resid, (size_t)qtl_cis_resid_capacity(G, n))); HIPCHK(dalloc(ws.bad, 1));
    HIPCHK(dalloc(ws.xbq, (size_t)qtl_xbq_capacity(rows, Pc))); HIPCHK(dalloc(ws.sums, (size_t)asc_sums_capacity(rows)));
    HIPCHK(dalloc(ws.info, (size_t)asc_info_capacity(rows)));
    HIPCHK(dalloc(ws.ws_r2, (size_t)qtl_cis_ws_capacity(wrows, P))); HIPCHK(dalloc(ws.ws_row, (size_t)qtl_cis_ws_capacity(wrows, P)));
    HIPCHK(dalloc(ws.ws_xb, (size_t)qtl_cis_wsxb_capacity(wrows, P)));
    HIPCHK(dalloc(ws.run_r2, (size_t)qtl_cis_run_capacity(P))); HIPCHK(dalloc(ws.run_row, (size_t)qtl_cis_run_capacity(P))); HIPCHK(dalloc(ws.run_xb, 1));
    HIPCHK(dalloc(ws.perm_r2, (size_t)qtl_cis_result_capacity(G, P))); HIPCHK(dalloc(ws.best, (size_t)qtl_cis_best_capacity(G)));
    HIPCHK(hipMemsetAsync(ws.Bt, 0, (size_t)qtl_cis_panel_capacity(N, P) * 4, st));   // excluded samples, pad samples and pad columns stay 0
    HIPCHK(hipMemcpyAsync(ws.Qt, Qt.data(), Qt.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ws.incw, incw.data(), incw.size() * 4, hipMemcpyHostToDevice, st));
    if (P > 0) HIPCHK(hipMemcpyAsync(ws.perm, perm, (size_t)P * (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ws.S, S32.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (Pc > 0) HIPCHK(hipMemcpyAsync(ws.Q, d.Q.data(), (size_t)Pc * (size_t)n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ws.resid, d.Yc.data(), (size_t)G * (size_t)n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(ws.bad, 0xff, 8, st));
    const double df = (double)(n - Pc - 2);
    {
        // the per-row pass over the union of the windows, as gpca_assoc_qtl runs it over its band
        ScopedTimer t(h, "assoc_qtl_cis_rows", 2.0 * (double)rows * (double)N * (double)asc_lpad(Lq), (double)rows * (double)N * (packed ? 0.25 : 1.0));
        if (launch_assoc(st, Gm, packed, ldr, h->d_pca_rows, N, ws.Qt, ws.incw, Lq, ulo, uhi, ws.xbq, ws.sums, ws.bad) != 0)
            return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
        HIPCHK(hipGetLastError());
        launch_assoc_finish(st, ws.xbq, ws.sums, nullptr, Pc > 0 ? 0 : 1, Lq, df, max_vif, rows, nullptr, ws.info);
        HIPCHK(hipGetLastError());
    }
    CHK(asc_check_genotypes(h, f, ws.bad, st));
    // liveness on the host, by the kernel's rule on the same f64 values: live [i] for kept row ulo + i, then its running count
    std::vector<double> info((size_t)asc_info_capacity(rows));
    HIPCHK(hipMemcpy(info.data(), ws.info, info.size() * 8, hipMemcpyDeviceToHost));
    std::vector<int64_t> nlive((size_t)rows + 1, 0);
    for (int64_t i = 0; i < rows; ++i) {
        const double nobs = info[(size_t)(4 * i)], xx = info[(size_t)(4 * i + 2)], sxx = info[(size_t)(4 * i + 3)];
        const bool dead = nobs == 0.0 || !(xx > 0.0) || sxx * max_vif < xx;
        nlive[(size_t)i + 1] = nlive[(size_t)i] + (dead ? 0 : 1);
    }
    for (int64_t g = 0; g < G; ++g) {
        const int64_t lo = win[2 * g], hi = win[2 * g + 1];
        if (hi > lo) n_var[g] = nlive[(size_t)(hi - ulo)] - nlive[(size_t)(lo - ulo)];
    }
    for (int64_t g = 0; g < G; ++g) {
        if (n_var[g] == 0) continue;
        const int64_t lo = win[2 * g], hi = win[2 * g + 1];
        {
            ScopedTimer t(h, "qtl_perm_panel", 4.0 * (double)P * (double)n * (double)Pc, 4.0 * (double)T * (double)n);
            launch_qtl_perm_panel(st, ws.resid + qtl_cis_resid_index(g, n, 0), ws.Q, Pc, n, ws.perm, P, ws.S, npad, ws.Bt);
            HIPCHK(hipGetLastError());
        }
        ScopedTimer t(h, "assoc_qtl_cis", 2.0 * (double)(hi - lo) * (double)N * (double)qtl_tpad(T), (double)(hi - lo) * (double)N * (packed ? 0.25 : 1.0));
        const int tw = qtl_strip_width(std::min(chunk_blocks, asc_row_blocks(hi - lo)), T, forced);
        for (int64_t r = lo; r < hi; r += chunk_blocks * kAscRows) {
            const int64_t re = std::min(hi, r + chunk_blocks * kAscRows);
            if (launch_assoc_qtl_cis(st, Gm, packed, ldr, h->d_pca_rows, N, ws.Bt, ws.incw, yy[(size_t)g], T, tw, ulo, r, re, ws.sums, ws.info,
                                     max_vif, ws.ws_r2, ws.ws_row, ws.ws_xb) != 0)
                return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
            HIPCHK(hipGetLastError());
            launch_assoc_qtl_cis_best(st, ws.ws_r2, ws.ws_row, ws.ws_xb, asc_row_blocks(re - r), T, r == lo, re == hi, ws.run_r2, ws.run_row, ws.run_xb,
                                      g, ws.perm_r2, ws.best);
            HIPCHK(hipGetLastError());
        }
    }
    // the results, once per call
    std::vector<double> pr((size_t)qtl_cis_result_capacity(G, P)), bs((size_t)qtl_cis_best_capacity(G));
    if (P > 0) HIPCHK(hipMemcpyAsync(pr.data(), ws.perm_r2, pr.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(bs.data(), ws.best, bs.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int64_t g = 0; g < G; ++g) {
        if (n_var[g] == 0) continue;                                                  // (its slots were never written)
        best_r2[g] = bs[(size_t)(3 * g)];
        best_row[g] = (int64_t)bs[(size_t)(3 * g + 2)];
        best_stat[3 * g] = bs[(size_t)(3 * g + 1)];
        best_stat[3 * g + 1] = info[(size_t)(4 * (best_row[g] - ulo) + 3)];
        best_stat[3 * g + 2] = yy[(size_t)g];
        if (P > 0) std::copy(pr.begin() + g * (int64_t)P, pr.begin() + (g + 1) * (int64_t)P, perm_r2 + g * (int64_t)P);
    }
    return GPCA_OK;
}

extern "C" int gpca_qtl_perm_panel(gpca_handle* h, const double* b, const double* Q, int32_t Pc, int64_t n, const uint32_t* perm, int32_t P,
                                   float* out) {
    if (!h) return GPCA_ERR_BAD_ARG;
    LOCK(h);
    static const std::string f("gpca_qtl_perm_panel");
    if (n < 1 || n >= ((int64_t)1 << 31)) return fail(h, GPCA_ERR_BAD_ARG, f + ": 1 <= n < 2^31 is required");
    if (Pc < 0 || Pc > kQtlMaxPc) return fail(h, GPCA_ERR_BAD_ARG, f + ": 0 <= Pc <= " + std::to_string(kQtlMaxPc) + " is required");
    if (P < 0 || P > kQtlCisMaxPerm) return fail(h, GPCA_ERR_BAD_ARG, f + ": P must lie in [0, 65535]");
    if (!b || (Pc > 0 && !Q) || (P > 0 && (!perm || !out))) return fail(h, GPCA_ERR_BAD_ARG, f + ": b, Q (Pc > 0), perm and out (P > 0) are required");
    if (P == 0) return GPCA_OK;
    const int64_t badrow = first_bad_perm_row(perm, P, n);
    if (badrow >= 0)
        return fail(h, GPCA_ERR_BAD_ARG, f + ": row " + std::to_string(badrow) + " of perm is not a permutation of 0 .. n - 1 (n = " + std::to_string(n) + ")");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = h->st;
    std::vector<double> Qt((size_t)Pc * (size_t)n);                                   // [Pc][n], as AscDesign holds it
    for (int64_t i = 0; i < n; ++i)
        for (int j = 0; j < Pc; ++j) Qt[(size_t)j * (size_t)n + (size_t)i] = Q[i * Pc + j];
    CisWs ws;
    const size_t cells = (size_t)(P + 1) * (size_t)n;
    HIPCHK(dalloc(ws.Bt, cells)); HIPCHK(dalloc(ws.perm, (size_t)P * (size_t)n)); HIPCHK(dalloc(ws.Q, Qt.size())); HIPCHK(dalloc(ws.resid, (size_t)n));
    HIPCHK(hipMemcpyAsync(ws.perm, perm, (size_t)P * (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (Pc > 0) HIPCHK(hipMemcpyAsync(ws.Q, Qt.data(), Qt.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ws.resid, b, (size_t)n * 8, hipMemcpyHostToDevice, st));
    {
        ScopedTimer t(h, "qtl_perm_panel", 4.0 * (double)P * (double)n * (double)Pc, 4.0 * (double)(P + 1) * (double)n);
        launch_qtl_perm_panel(st, ws.resid, ws.Q, Pc, n, ws.perm, P, nullptr, n, ws.Bt);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(out, ws.Bt + n, (size_t)P * (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GPCA_OK;
}

// Row p: a = 0 .. n - 1, then for step s = 0 .. n - 2 with i = n - 1 - s: r = word s & 3 of philox4x32-10(counter = (s >> 2, p, 0,
// GPCA_STREAM_QTL_PERM), key = the seed's low and high word), j = ((uint64) r (i + 1)) >> 32, swap a[i] and a[j].
extern "C" int gpca_qtl_perm_table(uint64_t seed, int64_t n, int32_t P, uint32_t* out) {
    if (n < 0 || n >= ((int64_t)1 << 32) || P < 0 || P > kQtlCisMaxPerm || (!out && n > 0 && P > 0)) return GPCA_ERR_BAD_ARG;
    for (int64_t p = 0; p < P; ++p) {
        uint32_t* a = out + p * n;
        for (int64_t i = 0; i < n; ++i) a[i] = (uint32_t)i;
        philox_out w{};
        for (int64_t s = 0; s + 1 < n; ++s) {
            if ((s & 3) == 0) w = philox4x32_10((uint32_t)(s >> 2), (uint32_t)p, 0u, GPCA_STREAM_QTL_PERM, (uint32_t)seed, (uint32_t)(seed >> 32));
            const int64_t i = n - 1 - s;
            const int64_t j = (int64_t)(((uint64_t)w.v[s & 3] * (uint64_t)(i + 1)) >> 32);
            std::swap(a[i], a[j]);
        }
    }
    return GPCA_OK;
}

namespace {
// digamma and trigamma for x > 0: the recurrence up to x >= 10, then the asymptotic series
double digamma(double x) {
    double r = 0.0;
    while (x < 10.0) { r -= 1.0 / x; x += 1.0; }
    const double f = 1.0 / (x * x);
    return r + std::log(x) - 0.5 / x -
           f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f * (1.0 / 132 - f * (691.0 / 32760 - f * (1.0 / 12)))))));
}
double trigamma(double x) {
    double r = 0.0;
    while (x < 10.0) { r += 1.0 / (x * x); x += 1.0; }
    const double f = 1.0 / (x * x);
    return r + 1.0 / x + 0.5 * f +
           (1.0 / x) * f * (1.0 / 6 - f * (1.0 / 30 - f * (1.0 / 42 - f * (1.0 / 30 - f * (5.0 / 66 - f * (691.0 / 2730 - f * (7.0 / 6)))))));
}
double log_beta(double a, double b) { return std::lgamma(a) + std::lgamma(b) - std::lgamma(a + b); }
// the continued fraction of the incomplete beta function (modified Lentz)
double beta_cf(double a, double b, double x) {
    const double tiny = 1e-300, eps = 1e-16;
    double c = 1.0, dd = 1.0 - (a + b) * x / (a + 1.0);
    if (std::fabs(dd) < tiny) dd = tiny;
    dd = 1.0 / dd;
    double hh = dd;
    for (int m = 1; m <= 10000; ++m) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((a + m2 - 1.0) * (a + m2));
        dd = 1.0 + aa * dd; if (std::fabs(dd) < tiny) dd = tiny;
        c = 1.0 + aa / c; if (std::fabs(c) < tiny) c = tiny;
        dd = 1.0 / dd; hh *= dd * c;
        aa = -(a + m) * (a + b + m) * x / ((a + m2) * (a + m2 + 1.0));
        dd = 1.0 + aa * dd; if (std::fabs(dd) < tiny) dd = tiny;
        c = 1.0 + aa / c; if (std::fabs(c) < tiny) c = tiny;
        dd = 1.0 / dd;
        const double del = dd * c;
        hh *= del;
        if (std::fabs(del - 1.0) < eps) break;
    }
    return hh;
}
// log I_x(a, b) from log x (x itself may underflow to 0: the fraction is then 1 and log(1 - x) = 0)
double log_betainc(double a, double b, double logx) {
    const double x = std::exp(logx);
    if (!(logx < 0.0)) return 0.0;
    if (x < (a + 1.0) / (a + b + 2.0))
        return a * logx + b * std::log1p(-x) - log_beta(a, b) - std::log(a) + std::log(beta_cf(a, b, x));
    const double y = 1.0 - x;                                                        // the other tail: 1 - I_{1-x}(b, a)
    const double lt = b * std::log1p(-x) + a * logx - log_beta(a, b) - std::log(b) + std::log(beta_cf(b, a, y));
    return std::log1p(-std::exp(lt));
}
const double kLn10 = 2.302585092994045684;
// -log10 of the two-sided Student p of r2 at d degrees of freedom
double r2_log10p(double r2, double d) {
    if (r2 >= 1.0) return INFINITY;
    return gpca_student_t_log10p(std::sqrt(d * r2 / (1.0 - r2)), d);
}
struct Moments { double m, v; };
Moments p_moments(const std::vector<double>& r2, double d, std::vector<double>* pv) {
    const double n = (double)r2.size();
    double s = 0.0;
    std::vector<double> local;
    std::vector<double>& p = pv ? *pv : local;
    p.resize(r2.size());
    for (size_t i = 0; i < r2.size(); ++i) { p[i] = std::pow(10.0, -r2_log10p(r2[i], d)); s += p[i]; }
    const double m = s / n;
    double ss = 0.0;
    for (double x : p) ss += (x - m) * (x - m);
    return Moments{m, ss / (n - 1.0)};
}
double shape1_mom(const Moments& q) { return q.m * (q.m * (1.0 - q.m) / q.v - 1.0); }
double shape2_mom(const Moments& q) { return (1.0 - q.m) * (q.m * (1.0 - q.m) / q.v - 1.0); }
}  // namespace

extern "C" int gpca_qtl_beta_approx(const double* perm_r2, int64_t P, double r2_nominal, double df, double* out, int32_t* status) {
    if (!out || P < 0 || (P > 0 && !perm_r2)) return GPCA_ERR_BAD_ARG;
    const double nan = std::nan("");
    for (int i = 0; i < 7; ++i) out[i] = nan;
    if (status) *status = 0;
    if (std::isnan(r2_nominal) || !(df >= 1.0) || !std::isfinite(df)) return GPCA_OK;
    std::vector<double> r2;
    r2.reserve((size_t)P);
    int64_t ge = 0;
    for (int64_t i = 0; i < P; ++i)
        if (!std::isnan(perm_r2[i])) { r2.push_back(perm_r2[i]); if (perm_r2[i] >= r2_nominal) ++ge; }
    out[0] = (1.0 + (double)ge) / ((double)r2.size() + 1.0);
    if (r2.size() < 10) return GPCA_OK;
    int32_t stt = 0;
    // (b) the root in d of log shape1_mom(d) = 0, by bisection on [1, 2 df] down to 1e-6 df
    auto fdf = [&](double d) { return std::log(shape1_mom(p_moments(r2, d, nullptr))); };
    double lo = 1.0, hi = 2.0 * df, true_df = df;
    double flo = fdf(lo), fhi = fdf(hi);
    if (std::isfinite(flo) && std::isfinite(fhi) && flo != 0.0 && fhi != 0.0 && (flo < 0.0) != (fhi < 0.0)) {
        while (hi - lo > 1e-6 * df) {
            const double mid = lo + 0.5 * (hi - lo), fm = fdf(mid);
            if (!std::isfinite(fm)) break;
            if ((fm < 0.0) == (flo < 0.0)) { lo = mid; flo = fm; } else hi = mid;
        }
        true_df = lo + 0.5 * (hi - lo);
    } else if (std::isfinite(flo) && flo == 0.0) true_df = lo;
    else if (std::isfinite(fhi) && fhi == 0.0) true_df = hi;
    else stt |= 1;
    // (c) the maximum-likelihood Beta fit of p(perm_r2, true_df): Newton with halving from the moment estimates
    std::vector<double> pv;
    const Moments q = p_moments(r2, true_df, &pv);
    const double a0 = shape1_mom(q), b0 = shape2_mom(q);
    double a = a0, b = b0;
    bool ok = std::isfinite(a0) && std::isfinite(b0) && a0 > 0.0 && b0 > 0.0;
    if (ok) {
        double l1 = 0.0, l2 = 0.0;
        for (double x : pv) { l1 += std::log(x); l2 += std::log1p(-x); }
        l1 /= (double)pv.size(); l2 /= (double)pv.size();
        ok = std::isfinite(l1) && std::isfinite(l2);
        auto resid = [&](double aa, double bb, double& g1, double& g2) {
            const double dab = digamma(aa + bb);
            g1 = digamma(aa) - dab - l1; g2 = digamma(bb) - dab - l2;
        };
        bool conv = false;
        for (int it = 0; ok && it < 100; ++it) {
            double g1, g2;
            resid(a, b, g1, g2);
            const double nrm = std::max(std::fabs(g1), std::fabs(g2));
            if (nrm <= 1e-13) { conv = true; break; }
            const double tab = trigamma(a + b), j11 = trigamma(a) - tab, j22 = trigamma(b) - tab, j12 = -tab;
            const double det = j11 * j22 - j12 * j12;
            if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) { ok = false; break; }
            const double da = (j22 * g1 - j12 * g2) / det, db = (j11 * g2 - j12 * g1) / det;
            double step = 1.0;
            bool moved = false;
            for (int hv = 0; hv < 60; ++hv, step *= 0.5) {
                const double na = a - step * da, nb = b - step * db;
                if (!(na > 0.0) || !(nb > 0.0)) continue;
                double h1, h2;
                resid(na, nb, h1, h2);
                if (std::max(std::fabs(h1), std::fabs(h2)) < nrm) { a = na; b = nb; moved = true; break; }
            }
            if (!moved) { conv = nrm <= 1e-10; break; }                              // (no descent left: at the rounding floor, or lost)
        }
        ok = ok && conv;
    }
    if (!ok) { a = a0; b = b0; stt |= 2; }
    out[1] = true_df; out[2] = a; out[3] = b; out[6] = a0;
    // (d), (e)
    out[4] = r2_log10p(r2_nominal, true_df);
    if (a > 0.0 && b > 0.0 && std::isfinite(a) && std::isfinite(b))
        out[5] = std::isinf(out[4]) ? INFINITY : -log_betainc(a, b, -out[4] * kLn10) / kLn10;
    if (status) *status = stt;
    return GPCA_OK;
}
