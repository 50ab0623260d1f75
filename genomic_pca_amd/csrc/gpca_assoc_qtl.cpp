// gpca_assoc_qtl / gpca_qtl_stats (include/gpca.h section a24): the many-trait QTL scan.  The host step is gpca_assoc_linear's
// (asc_design_host, gpca_assoc.cpp) on all T columns; the covariate basis goes through k_assoc once for the per-row sums, the covariate
// products and rowinfo (launch_assoc, launch_assoc_finish); k_assoc_qtl (assoc_qtl.hip) then multiplies every row block by strips of the
// trait panel and keeps the hits and the workgroups' bests, a launch per qtl_chunk_blocks(T) row blocks, each followed by the fold of
// its bests (k_assoc_qtl_best).  The records are sorted by (row, trait) here.  The call has its own workspace, allocated and freed per
// call, and reads nothing of the handle's state but the genotypes and the list of kept rows.
#include "gpca_internal.h"

#include <numeric>

using namespace gpca;

#pragma clang fp contract(off)

namespace {
struct QtlWs {
    float *Bt = nullptr, *Qt = nullptr;
    unsigned *incw = nullptr, *sums = nullptr, *hit_count = nullptr, *hit_index = nullptr;
    double *yy = nullptr, *xbq = nullptr, *info = nullptr, *hit_value = nullptr, *ws_r2 = nullptr, *best_r2 = nullptr;
    long long *ws_row = nullptr, *best_row = nullptr;
    unsigned long long *bad = nullptr, *counter = nullptr;
    ~QtlWs() {
        dfree(Bt); dfree(Qt); dfree(incw); dfree(sums); dfree(hit_count); dfree(hit_index); dfree(yy); dfree(xbq); dfree(info);
        dfree(hit_value); dfree(ws_r2); dfree(best_r2); dfree(ws_row); dfree(best_row); dfree(bad); dfree(counter);
    }
};
}  // namespace

extern "C" int gpca_assoc_qtl(gpca_handle* h, const double* Y, int64_t T, const double* C, int32_t Pc, const uint8_t* include, double max_vif,
                              double r2_min, int64_t row0, int64_t row1, double* rowinfo, double* yy_out, uint32_t* hit_count,
                              uint32_t* hit_index, double* hit_value, int64_t cap, int64_t* n_found, double* best_r2, int64_t* best_row) {
    if (!h) return GPCA_ERR_BAD_ARG;
    LOCK(h);
    static const std::string f("gpca_assoc_qtl");
    const char* out_err = !hit_count ? "hit_count is required" : !n_found ? "n_found is required"
                          : (best_r2 == nullptr) != (best_row == nullptr) ? "best_r2 and best_row go together: both or neither" : nullptr;
    const char* late_err = !(r2_min >= 0.0 && r2_min <= 1.0) ? "r2_min must lie in [0, 1]" : cap < 0 ? "cap must be at least 0"
                           : cap > 0 && (!hit_index || !hit_value) ? "hit_index and hit_value are required when cap > 0" : nullptr;
    CHK(asc_check_call(h, f, T >= 1 && T <= kQtlMaxTraits && Pc >= 0 && Pc <= kQtlMaxPc,
                       "1 <= T <= " + std::to_string(kQtlMaxTraits) + " and 0 <= Pc <= " + std::to_string(kQtlMaxPc), Y, C, Pc, out_err, row0, row1,
                       max_vif, late_err));
    const int64_t N = h->N, npad = asc_npad(N);
    if (row1 > ((int64_t)1 << 32)) return fail(h, GPCA_ERR_BAD_ARG, f + ": a kept row of the band does not fit the 32-bit record");
    AscDesign d;
    std::vector<unsigned> incw; std::vector<double> yy;
    CHK(asc_design_host(h, f, Y, T, C, Pc, include, d, incw, yy));
    const int64_t n_inc = (int64_t)d.S.size();
    const int64_t rows = row1 - row0;
    *n_found = 0;
    if (yy_out) std::copy(yy.begin(), yy.end(), yy_out);
    if (best_r2) for (int64_t t = 0; t < T; ++t) { best_r2[t] = std::nan(""); best_row[t] = -1; }
    if (rows == 0) return GPCA_OK;
    std::fill(hit_count, hit_count + rows, 0u);
    if (asc_row_blocks(rows) >= ((int64_t)1 << 31)) return fail(h, GPCA_ERR_BAD_ARG, f + ": the band makes 2^31 or more workgroups: ask for fewer rows");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->st));
    CHK(preflight_device_memory(h, f.c_str(), "the band needs", qtl_call_bytes(N, rows, T, Pc, cap) + (double)(64 << 20)));
    int64_t forced = 0;
    if (const char* e = std::getenv("GPCA_QTL_TW")) {                                 // read per call: the tests' way to every strip edge
        forced = std::strtoll(e, nullptr, 10);
        if (forced < 1) forced = 1;
    }
    const int64_t chunk_blocks = qtl_wsbest_blocks(rows, T);
    const int tw = qtl_strip_width(chunk_blocks, T, forced);
    const int Lq = qtl_cov_cols(Pc);

    // the panels: the traits [qtl_tpad(T)][npad], the covariate basis [asc_lpad(Lq)][npad] (Pc = 0: a column of zeros), yy (1 past T)
    std::vector<float> Bt((size_t)qtl_b_capacity(N, T), 0.0f), Qt((size_t)qtl_q_capacity(N, Pc), 0.0f);
    asc_design_rows(d, d.Yc, T, npad, Bt.data());
    asc_design_rows(d, d.Q, Pc, npad, Qt.data());
    std::vector<double>().swap(d.Yc);
    std::vector<double> yyp((size_t)qtl_yy_capacity(T), 1.0);
    std::copy(yy.begin(), yy.end(), yyp.begin());

    const bool packed = h->storage == GPCA_STORE_2BIT;
    const auto [G, ldr] = panel_rows(h, resident_view(h));
    hipStream_t st = h->st;
    QtlWs ws;
    HIPCHK(dalloc(ws.Bt, Bt.size())); HIPCHK(dalloc(ws.Qt, Qt.size())); HIPCHK(dalloc(ws.incw, incw.size())); HIPCHK(dalloc(ws.yy, yyp.size()));
    HIPCHK(dalloc(ws.bad, 1)); HIPCHK(dalloc(ws.counter, 1));
    HIPCHK(dalloc(ws.xbq, (size_t)qtl_xbq_capacity(rows, Pc))); HIPCHK(dalloc(ws.sums, (size_t)asc_sums_capacity(rows)));
    HIPCHK(dalloc(ws.info, (size_t)asc_info_capacity(rows))); HIPCHK(dalloc(ws.hit_count, (size_t)qtl_hitcount_capacity(rows)));
    HIPCHK(dalloc(ws.hit_index, (size_t)qtl_rec_capacity(cap))); HIPCHK(dalloc(ws.hit_value, (size_t)qtl_rec_capacity(cap)));
    HIPCHK(dalloc(ws.ws_r2, (size_t)qtl_wsbest_capacity(rows, T))); HIPCHK(dalloc(ws.ws_row, (size_t)qtl_wsbest_capacity(rows, T)));
    HIPCHK(dalloc(ws.best_r2, (size_t)T)); HIPCHK(dalloc(ws.best_row, (size_t)T));
    HIPCHK(hipMemcpyAsync(ws.Bt, Bt.data(), Bt.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ws.Qt, Qt.data(), Qt.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ws.incw, incw.data(), incw.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ws.yy, yyp.data(), yyp.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(ws.bad, 0xff, 8, st));
    HIPCHK(hipMemsetAsync(ws.counter, 0, 8, st));
    HIPCHK(hipMemsetAsync(ws.hit_count, 0, (size_t)rows * 4, st));
    // the running best: r2 = -1 (bit pattern of -1.0), row = -1
    std::vector<double> b2((size_t)T, -1.0);
    std::vector<long long> bw((size_t)T, -1);
    HIPCHK(hipMemcpyAsync(ws.best_r2, b2.data(), (size_t)T * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ws.best_row, bw.data(), (size_t)T * 8, hipMemcpyHostToDevice, st));
    const double df = (double)(n_inc - Pc - 2);
    {
        // the per-row pass: the covariate products, the sums and rowinfo (sxx = xx - sum_j xb_ij^2, j ascending: a12's, whose covariate
        // columns carry the same bits wherever they sit in the panel; with Pc = 0 the one column is taken as a trait, so sxx = xx - 0)
        ScopedTimer t(h, "assoc_qtl_rows", 2.0 * (double)rows * (double)N * (double)asc_lpad(Lq), (double)rows * (double)N * (packed ? 0.25 : 1.0));
        if (launch_assoc(st, G, packed, ldr, h->d_pca_rows, N, ws.Qt, ws.incw, Lq, row0, row1, ws.xbq, ws.sums, ws.bad) != 0)
            return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
        HIPCHK(hipGetLastError());
        launch_assoc_finish(st, ws.xbq, ws.sums, nullptr, Pc > 0 ? 0 : 1, Lq, df, max_vif, rows, nullptr, ws.info);
        HIPCHK(hipGetLastError());
    }
    CHK(asc_check_genotypes(h, f, ws.bad, st));
    {
        ScopedTimer t(h, "assoc_qtl", 2.0 * (double)rows * (double)N * (double)qtl_tpad(T), (double)rows * (double)N * (packed ? 0.25 : 1.0));
        for (int64_t r = row0; r < row1; r += chunk_blocks * kAscRows) {
            const int64_t re = std::min(row1, r + chunk_blocks * kAscRows);
            if (launch_assoc_qtl(st, G, packed, ldr, h->d_pca_rows, N, ws.Bt, ws.incw, ws.yy, T, tw, row0, r, re, ws.sums, ws.info, max_vif,
                                 r2_min, ws.hit_count, ws.hit_index, ws.hit_value, cap, ws.counter, ws.ws_r2, ws.ws_row) != 0)
                return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
            HIPCHK(hipGetLastError());
            launch_assoc_qtl_best(st, ws.ws_r2, ws.ws_row, asc_row_blocks(re - r), T, ws.best_r2, ws.best_row);
            HIPCHK(hipGetLastError());
        }
    }
    unsigned long long found = 0;
    HIPCHK(hipMemcpyAsync(&found, ws.counter, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hit_count, ws.hit_count, (size_t)rows * 4, hipMemcpyDeviceToHost, st));
    if (rowinfo) HIPCHK(hipMemcpyAsync(rowinfo, ws.info, (size_t)asc_info_capacity(rows) * 8, hipMemcpyDeviceToHost, st));
    if (best_r2) {
        HIPCHK(hipMemcpyAsync(b2.data(), ws.best_r2, (size_t)T * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(bw.data(), ws.best_row, (size_t)T * 8, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    *n_found = (int64_t)found;
    if (best_r2)
        for (int64_t t = 0; t < T; ++t) {
            best_row[t] = (int64_t)bw[(size_t)t];
            best_r2[t] = bw[(size_t)t] < 0 ? std::nan("") : b2[(size_t)t];
        }
    if ((int64_t)found <= cap && found > 0) {
        // the records in the order the waves appended them -> ascending (row, trait)
        const size_t n = (size_t)found;
        std::vector<uint32_t> hi(2 * n);
        std::vector<double> hv(2 * n);
        HIPCHK(hipMemcpy(hi.data(), ws.hit_index, 2 * n * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(hv.data(), ws.hit_value, 2 * n * 8, hipMemcpyDeviceToHost));
        std::vector<size_t> order(n);
        std::iota(order.begin(), order.end(), (size_t)0);
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
            return hi[2 * a] != hi[2 * b] ? hi[2 * a] < hi[2 * b] : hi[2 * a + 1] < hi[2 * b + 1];
        });
        for (size_t i = 0; i < n; ++i) {
            const size_t s = order[i];
            hit_index[2 * i] = hi[2 * s]; hit_index[2 * i + 1] = hi[2 * s + 1];
            hit_value[2 * i] = hv[2 * s]; hit_value[2 * i + 1] = hv[2 * s + 1];
        }
    }
    return GPCA_OK;
}

// a12's step 3 for one pair: beta = xb / sxx, rss = yy - xb beta, se = sqrt(rss / df / sxx), t = beta / se; NaN when rss <= 0
extern "C" void gpca_qtl_stats(double xb, double sxx, double yy, double df, double* out) {
    if (!out) return;
    const double beta = xb / sxx;
    const double rss = yy - xb * beta;
    const double se = std::sqrt(rss / df / sxx);
    const bool ok = rss > 0.0;
    const double nan = std::nan("");
    out[0] = ok ? beta : nan; out[1] = ok ? se : nan; out[2] = ok ? beta / se : nan;
}

// the smallest t >= 0 whose two-sided -log10 p at df degrees of freedom reaches log10p: bisection on gpca_student_t_log10p (monotone in
// t) down to neighbouring doubles.  0 for log10p <= 0; NaN for a NaN argument or df <= 0; +inf when no finite t reaches it.
extern "C" double gpca_qtl_t_min(double log10p, double df) {
    if (std::isnan(log10p) || !(df > 0.0) || !std::isfinite(df)) return std::nan("");
    if (!(log10p > 0.0)) return 0.0;
    double lo = 0.0, hi = 1.0;
    while (gpca_student_t_log10p(hi, df) < log10p) {
        lo = hi; hi *= 2.0;
        if (std::isinf(hi)) return INFINITY;
    }
    while (std::nextafter(lo, hi) < hi) {
        const double mid = lo + 0.5 * (hi - lo);
        if (gpca_student_t_log10p(mid, df) < log10p) lo = mid; else hi = mid;
    }
    return hi;
}
