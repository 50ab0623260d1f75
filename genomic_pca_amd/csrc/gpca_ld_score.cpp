// gpca_ld_score, gpca_ld_score_total, gpca_ldsc_fit (include/gpca.h section a19).  The device call runs gpca_ld_window's two sweep
// launches as they are (launch_ld_vec, launch_ld) and reduces their product planes to one integer sum per row on the device
// (k_ld_score in ld.hip): no pair is copied to the host.  Its workspace is allocated and freed per call, and it reads nothing of the
// handle's state but the genotypes and the list of kept rows.  The two host rules take no handle.
#include "gpca_internal.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace gpca;

namespace {
struct LdScoreWs {
    int* W = nullptr;
    unsigned* stat = nullptr;
    unsigned long long* bad = nullptr;
    int64_t* win_end = nullptr;
    long long* acc = nullptr;
    int* partners = nullptr;
    ~LdScoreWs() { dfree(W); dfree(stat); dfree(bad); dfree(win_end); dfree(acc); dfree(partners); }
};
}  // namespace

extern "C" int gpca_ld_score(gpca_handle* h, int64_t row0, int64_t row1, const int64_t* win_end, int32_t wmax, int32_t flags, int64_t* score,
                             int32_t* partners) {
    if (!h) return GPCA_ERR_BAD_ARG;
    LOCK(h);
    if (!have_genotypes(h)) return fail(h, GPCA_ERR_STATE, "gpca_ld_score: no genotypes resident");
    if (h->sm.on)
        return fail(h, GPCA_ERR_STATE, "gpca_ld_score: the handle streams its matrix in panels; a window crosses panel boundaries and needs a halo of wmax rows, which is not implemented");
    if (multi_rank(h))
        return fail(h, GPCA_ERR_STATE, "gpca_ld_score: the handle holds a shard of the rows; a window crosses shard boundaries and needs a halo of wmax rows, which is not implemented");
    if (!h->have_stats) return fail(h, GPCA_ERR_STATE, "gpca_ld_score: no standardisation: run gpca_snp_stats or gpca_set_standardization first");
    const int64_t K = h->n_pca, N = h->N;
    if (K == 0) return fail(h, GPCA_ERR_STATE, "gpca_ld_score: no kept row (the keep mask is empty)");
    if (!score) return fail(h, GPCA_ERR_BAD_ARG, "gpca_ld_score: score is NULL");
    if (flags & ~GPCA_LDSCORE_UNBIASED) return fail(h, GPCA_ERR_BAD_ARG, "gpca_ld_score: unknown flag bits");
    if (row0 < 0 || row1 < row0 || row1 > K)
        return fail(h, GPCA_ERR_BAD_ARG, "gpca_ld_score: rows must satisfy 0 <= row0 <= row1 <= K (K = " + std::to_string(K) + " kept rows)");
    if (wmax < 1) return fail(h, GPCA_ERR_BAD_ARG, "gpca_ld_score: wmax must be at least 1");
    if (wmax > kLdScoreMaxWmax) return fail(h, GPCA_ERR_BAD_ARG, "gpca_ld_score: wmax must be at most 2^20 (the 64-bit sums of 2 wmax pairs)");
    if (4 * N >= ((int64_t)1 << 31)) return fail(h, GPCA_ERR_BAD_ARG, "gpca_ld_score: 2^29 or more samples (the sums of squares are 32-bit)");
    const int64_t rows = row1 - row0;
    if (rows == 0) return GPCA_OK;
    if (!win_end) return fail(h, GPCA_ERR_BAD_ARG, "gpca_ld_score: win_end is required");
    int64_t hi = row1, weff = 0;
    for (int64_t t = 0; t < rows; ++t) {
        const int64_t i = row0 + t, we = win_end[t];
        if (we < i + 1 || we > std::min(K, i + 1 + (int64_t)wmax))
            return fail(h, GPCA_ERR_BAD_ARG, "gpca_ld_score: win_end of row " + std::to_string(i) + " is " + std::to_string(we) +
                                                 ": it must lie in [row + 1, min(K, row + 1 + wmax)]");
        hi = std::max(hi, we);
        weff = std::max(weff, we - i - 1);
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->st));
    const bool packed = h->storage == GPCA_STORE_2BIT;
    const auto [G, ldr] = panel_rows(h, resident_view(h));
    const int64_t span = ld_score_span(K, row0, row1, wmax);

    // preflight: everything the call allocates on the device, before any allocation
    const double slots = (double)rows * (double)wmax;
    const double need = 4.0 * kLdProducts * slots + 8.0 * (double)rows + 12.0 * (double)(hi - row0) + 12.0 * (double)span + (double)(64 << 20);
    CHK(preflight_device_memory(h, "gpca_ld_score", "the band needs", need));
    if (ld_row_blocks(rows) * ld_col_chunks(weff) >= ((int64_t)1 << 31) || ld_score_grid(rows, weff) >= ((int64_t)1 << 31))
        return fail(h, GPCA_ERR_BAD_ARG, "gpca_ld_score: the band makes 2^31 or more workgroups: ask for fewer rows");

    LdScoreWs ws;
    hipStream_t st = h->st;
    const size_t nacc = (size_t)ld_score_acc_capacity(K, row0, row1, wmax), npart = (size_t)ld_score_partners_capacity(K, row0, row1, wmax);
    HIPCHK(dalloc(ws.W, (size_t)ld_ws_capacity(rows, wmax)));
    HIPCHK(dalloc(ws.stat, (size_t)ld_stat_capacity(row0, hi)));
    HIPCHK(dalloc(ws.bad, 1));
    HIPCHK(dalloc(ws.win_end, (size_t)rows));
    HIPCHK(dalloc(ws.acc, nacc));
    HIPCHK(dalloc(ws.partners, npart));
    HIPCHK(hipMemcpyAsync(ws.win_end, win_end, (size_t)rows * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(ws.bad, 0xff, 8, st));
    HIPCHK(hipMemsetAsync(ws.W, 0, (size_t)ld_ws_capacity(rows, wmax) * 4, st));
    HIPCHK(hipMemsetAsync(ws.acc, 0, nacc * 8, st));
    HIPCHK(hipMemsetAsync(ws.partners, 0, npart * 4, st));
    {
        const double tiles = (double)ld_row_blocks(rows) * 2.0 * ((double)weff / 32.0 + 1.0);
        ScopedTimer t(h, "ld", 2.0 * 32.0 * 32.0 * (double)N * tiles, (double)(hi - row0) * (double)N * (packed ? 0.25 : 1.0));
        launch_ld_vec(st, G, packed, ldr, h->d_pca_rows, N, row0, hi, ws.stat, ws.bad);
        launch_ld(st, G, packed, ldr, h->d_pca_rows, K, N, row0, row1, ws.win_end, wmax, (int)weff, ws.W);
        HIPCHK(hipGetLastError());
    }
    CHK(asc_check_genotypes(h, "gpca_ld_score", ws.bad, st));
    {
        ScopedTimer t(h, "ld_score", 0.0, 4.0 * kLdProducts * (double)rows * (double)weff);
        launch_ld_score(st, ws.W, ws.stat, N, row0, row1, hi, ws.win_end, wmax, (int)weff, (flags & GPCA_LDSCORE_UNBIASED) ? 1 : 0, ws.acc, ws.partners);
        HIPCHK(hipGetLastError());
    }
    static_assert(sizeof(long long) == sizeof(int64_t), "acc is int64");
    HIPCHK(hipMemcpyAsync(score, ws.acc, (size_t)span * 8, hipMemcpyDeviceToHost, st));
    if (partners) HIPCHK(hipMemcpyAsync(partners, ws.partners, (size_t)span * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GPCA_OK;
}

extern "C" int gpca_ld_score_total(const int64_t* acc, int64_t K, double* l2) {
    if (K < 0 || (K > 0 && (!acc || !l2))) return GPCA_ERR_BAD_ARG;
    for (int64_t i = 0; i < K; ++i) l2[i] = 1.0 + (double)acc[i] * (1.0 / 1099511627776.0);
    return GPCA_OK;
}

// ---- LD-score regression (a19): every step in f64, in the order the header states, no fused multiply-add --------------------------------
namespace {
#pragma clang fp contract(off)
struct LdscSums { double w = 0, wl = 0, wll = 0, wc = 0, wlc = 0; };
inline LdscSums ldsc_minus(const LdscSums& a, const LdscSums& b) {
    LdscSums r;
    r.w = a.w - b.w; r.wl = a.wl - b.wl; r.wll = a.wll - b.wll; r.wc = a.wc - b.wc; r.wlc = a.wlc - b.wlc;
    return r;
}
// the 2 x 2 weighted least squares of chi2 on (1, l) by its determinant; false when the determinant is <= 0 or not finite
inline bool ldsc_solve(const LdscSums& s, double& a, double& b) {
    const double det = s.w * s.wll - s.wl * s.wl;
    if (!(det > 0.0) || !std::isfinite(det)) return false;
    a = (s.wll * s.wc - s.wl * s.wlc) / det;
    b = (s.w * s.wlc - s.wl * s.wc) / det;
    return true;
}
inline double ldsc_clamp01(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }
}  // namespace

extern "C" int gpca_ldsc_fit(const double* chi2, const double* ell, const double* w_ell, int64_t m, double n_samples, double M, int32_t n_blocks,
                             double chi2_max, double* out) {
#pragma clang fp contract(off)
    if (!chi2 || !ell || !out || m < 0) return GPCA_ERR_BAD_ARG;
    if (!(n_samples > 0.0) || !(M > 0.0) || !std::isfinite(n_samples) || !std::isfinite(M)) return GPCA_ERR_BAD_ARG;
    const double* wl_in = w_ell ? w_ell : ell;
    std::vector<double> c, l, wl;
    for (int64_t j = 0; j < m; ++j) {
        if (!std::isfinite(chi2[j]) || !std::isfinite(ell[j]) || !std::isfinite(wl_in[j])) continue;
        if (chi2_max > 0.0 && !(chi2[j] <= chi2_max)) continue;
        c.push_back(chi2[j]);
        l.push_back(std::max(ell[j], 1.0));
        wl.push_back(std::max(wl_in[j], 1.0));
    }
    const int64_t mu = (int64_t)c.size();
    const int64_t B = std::min<int64_t>(n_blocks, mu);
    if (B < 2 || mu < 3) return GPCA_ERR_BAD_ARG;
    double sc = 0.0, sl = 0.0;
    for (int64_t j = 0; j < mu; ++j) { sc += c[(size_t)j]; sl += l[(size_t)j]; }
    const double mean_c = sc / (double)mu, mean_l = sl / (double)mu;
    double a = 1.0, hh = ldsc_clamp01((M * (mean_c - 1.0)) / (n_samples * mean_l));

    std::vector<double> w((size_t)mu);
    std::vector<LdscSums> blk((size_t)B);
    LdscSums tot;
    auto weights = [&]() {
        const double nh = n_samples * ldsc_clamp01(hh);
        for (int64_t j = 0; j < mu; ++j) {
            const double t = a + (nh * l[(size_t)j]) / M;
            w[(size_t)j] = 1.0 / ((wl[(size_t)j] * 2.0) * (t * t));
        }
    };
    auto sums = [&]() {
        tot = LdscSums();
        for (int64_t k = 0; k < B; ++k) {
            LdscSums s;
            const int64_t j0 = mu * k / B, j1 = mu * (k + 1) / B;
            for (int64_t j = j0; j < j1; ++j) {
                const double wj = w[(size_t)j], lj = l[(size_t)j], cj = c[(size_t)j];
                s.w += wj; s.wl += wj * lj; s.wll += (wj * lj) * lj; s.wc += wj * cj; s.wlc += (wj * lj) * cj;
            }
            blk[(size_t)k] = s;
            tot.w += s.w; tot.wl += s.wl; tot.wll += s.wll; tot.wc += s.wc; tot.wlc += s.wlc;
        }
    };
    double b = 0.0;
    for (int round = 0; round < 3; ++round) {
        weights();
        sums();
        if (!ldsc_solve(tot, a, b)) return GPCA_ERR_BAD_ARG;
        hh = (b * M) / n_samples;
    }
    // delete-one jackknife over the blocks, with the final weights
    std::vector<double> pa((size_t)B), ph((size_t)B);
    for (int64_t k = 0; k < B; ++k) {
        double ak, bk;
        if (!ldsc_solve(ldsc_minus(tot, blk[(size_t)k]), ak, bk)) return GPCA_ERR_BAD_ARG;
        const double hk = (bk * M) / n_samples;
        pa[(size_t)k] = (double)B * a - (double)(B - 1) * ak;
        ph[(size_t)k] = (double)B * hh - (double)(B - 1) * hk;
    }
    auto jack_se = [&](const std::vector<double>& p) {
        double s = 0.0;
        for (double v : p) s += v;
        const double mean = s / (double)B;
        double q = 0.0;
        for (double v : p) q += (v - mean) * (v - mean);
        return std::sqrt((q / (double)(B - 1)) / (double)B);
    };
    const double se_a = jack_se(pa), se_h = jack_se(ph);
    std::vector<double> sorted(c);
    std::sort(sorted.begin(), sorted.end());
    const double med = (mu & 1) ? sorted[(size_t)(mu / 2)] : 0.5 * (sorted[(size_t)(mu / 2 - 1)] + sorted[(size_t)(mu / 2)]);
    const double nan = std::nan("");
    out[0] = (double)mu;
    out[1] = mean_c;
    out[2] = med / 0.4549364231195724;
    out[3] = a; out[4] = se_a;
    out[5] = hh; out[6] = se_h;
    out[7] = mean_c > 1.0 ? (a - 1.0) / (mean_c - 1.0) : nan;
    out[8] = mean_c > 1.0 ? se_a / (mean_c - 1.0) : nan;
    out[9] = (double)B;
    return GPCA_OK;
}
