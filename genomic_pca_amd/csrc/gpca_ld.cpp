// gpca_ld_window (include/gpca.h section a10): the six pair counts and r^2 of every kept row of a band against the kept rows of its
// window.  One vector pass for the per-row sums and the dosage check, one banded sweep of the resident matrix on the matrix cores
// (ld.hip), one pass that turns the counts into r^2 and the threshold bits.  The call has its own workspace, allocated and freed per
// call, and reads nothing of the handle's state but the genotypes and the list of kept rows.
#include "gpca_internal.h"

using namespace gpca;

namespace {
struct LdWs {
    int* W = nullptr;
    unsigned* stat = nullptr;
    unsigned long long* bad = nullptr;
    int64_t* win_end = nullptr;
    double* r2 = nullptr;
    int* counts = nullptr;
    unsigned long long* above = nullptr;
    ~LdWs() { dfree(W); dfree(stat); dfree(bad); dfree(win_end); dfree(r2); dfree(counts); dfree(above); }
};
}  // namespace

extern "C" int gpca_ld_window(gpca_handle* h, int64_t row0, int64_t row1, const int64_t* win_end, int32_t wmax, double threshold, double* r2,
                              int32_t* counts, uint64_t* above) {
    if (!h) return GPCA_ERR_BAD_ARG;
    LOCK(h);
    if (!have_genotypes(h)) return fail(h, GPCA_ERR_STATE, "gpca_ld_window: no genotypes resident");
    if (h->sm.on)
        return fail(h, GPCA_ERR_STATE, "gpca_ld_window: the handle streams its matrix in panels; a window crosses panel boundaries and needs a halo of wmax rows, which is not implemented");
    if (multi_rank(h))
        return fail(h, GPCA_ERR_STATE, "gpca_ld_window: the handle holds a shard of the rows; a window crosses shard boundaries and needs a halo of wmax rows, which is not implemented");
    if (!h->have_stats) return fail(h, GPCA_ERR_STATE, "gpca_ld_window: no standardisation: run gpca_snp_stats or gpca_set_standardization first");
    const int64_t K = h->n_pca, N = h->N;
    if (K == 0) return fail(h, GPCA_ERR_STATE, "gpca_ld_window: no kept row (the keep mask is empty)");
    if (!r2 && !counts && !above) return fail(h, GPCA_ERR_BAD_ARG, "gpca_ld_window: r2, counts and above are all NULL");
    if (row0 < 0 || row1 < row0 || row1 > K)
        return fail(h, GPCA_ERR_BAD_ARG, "gpca_ld_window: rows must satisfy 0 <= row0 <= row1 <= K (K = " + std::to_string(K) + " kept rows)");
    if (wmax < 1) return fail(h, GPCA_ERR_BAD_ARG, "gpca_ld_window: wmax must be at least 1");
    if (above && !std::isfinite(threshold)) return fail(h, GPCA_ERR_BAD_ARG, "gpca_ld_window: threshold must be finite");
    if (4 * N >= ((int64_t)1 << 31)) return fail(h, GPCA_ERR_BAD_ARG, "gpca_ld_window: 2^29 or more samples (the sums of squares are 32-bit)");
    const int64_t rows = row1 - row0;
    if (rows == 0) return GPCA_OK;
    if (!win_end) return fail(h, GPCA_ERR_BAD_ARG, "gpca_ld_window: win_end is required");
    int64_t hi = row1, weff = 0;
    for (int64_t t = 0; t < rows; ++t) {
        const int64_t i = row0 + t, we = win_end[t];
        if (we < i + 1 || we > std::min(K, i + 1 + (int64_t)wmax))
            return fail(h, GPCA_ERR_BAD_ARG, "gpca_ld_window: win_end of row " + std::to_string(i) + " is " + std::to_string(we) +
                                                 ": it must lie in [row + 1, min(K, row + 1 + wmax)]");
        hi = std::max(hi, we);
        weff = std::max(weff, we - i - 1);
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->st));
    const bool packed = h->storage == GPCA_STORE_2BIT;
    const auto [G, ldr] = panel_rows(h, resident_view(h));

    // preflight: everything the call allocates on the device, before any allocation
    const double slots = (double)rows * (double)wmax;
    const double need = 4.0 * kLdProducts * slots + (r2 ? 8.0 * slots : 0.0) + (counts ? 24.0 * slots : 0.0) +
                        (above ? 8.0 * (double)rows * (double)ld_above_words(wmax) : 0.0) + 8.0 * (double)rows + 12.0 * (double)(hi - row0) +
                        (double)(64 << 20);
    CHK(preflight_device_memory(h, "gpca_ld_window", "the band needs", need));
    const int64_t nblocks = ld_row_blocks(rows) * ld_col_chunks(weff);
    if (nblocks >= ((int64_t)1 << 31) || rows * ((ld_above_words(wmax) + 3) / 4) >= ((int64_t)1 << 31))
        return fail(h, GPCA_ERR_BAD_ARG, "gpca_ld_window: the band makes 2^31 or more workgroups: ask for fewer rows");

    LdWs ws;
    hipStream_t st = h->st;
    const size_t nslots = (size_t)rows * (size_t)wmax, nab = (size_t)ld_above_capacity(rows, wmax);
    HIPCHK(dalloc(ws.W, (size_t)ld_ws_capacity(rows, wmax)));
    HIPCHK(dalloc(ws.stat, (size_t)ld_stat_capacity(row0, hi)));
    HIPCHK(dalloc(ws.bad, 1));
    HIPCHK(dalloc(ws.win_end, (size_t)rows));
    if (r2) HIPCHK(dalloc(ws.r2, (size_t)ld_r2_capacity(rows, wmax)));
    if (counts) HIPCHK(dalloc(ws.counts, (size_t)ld_counts_capacity(rows, wmax)));
    if (above) HIPCHK(dalloc(ws.above, nab));
    HIPCHK(hipMemcpyAsync(ws.win_end, win_end, (size_t)rows * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(ws.bad, 0xff, 8, st));
    HIPCHK(hipMemsetAsync(ws.W, 0, (size_t)ld_ws_capacity(rows, wmax) * 4, st));
    {
        const double tiles = (double)ld_row_blocks(rows) * 2.0 * ((double)weff / 32.0 + 1.0);
        ScopedTimer t(h, "ld", 2.0 * 32.0 * 32.0 * (double)N * tiles, (double)(hi - row0) * (double)N * (packed ? 0.25 : 1.0));
        launch_ld_vec(st, G, packed, ldr, h->d_pca_rows, N, row0, hi, ws.stat, ws.bad);
        launch_ld(st, G, packed, ldr, h->d_pca_rows, K, N, row0, row1, ws.win_end, wmax, (int)weff, ws.W);
        HIPCHK(hipGetLastError());
    }
    CHK(asc_check_genotypes(h, "gpca_ld_window", ws.bad, st));
    launch_ld_finish(st, ws.W, ws.stat, N, row0, row1, ws.win_end, wmax, threshold, ws.r2, ws.counts, ws.above);
    HIPCHK(hipGetLastError());
    if (r2) HIPCHK(hipMemcpyAsync(r2, ws.r2, nslots * 8, hipMemcpyDeviceToHost, st));
    if (counts) HIPCHK(hipMemcpyAsync(counts, ws.counts, nslots * 24, hipMemcpyDeviceToHost, st));
    if (above) HIPCHK(hipMemcpyAsync(above, ws.above, nab * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GPCA_OK;
}
