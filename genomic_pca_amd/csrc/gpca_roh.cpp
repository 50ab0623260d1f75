// gpca_roh / gpca_roh_select (include/gpca.h section a20): runs of homozygosity per sample over the kept rows of a band, and the host
// rule that keeps a record by its length in bp and its SNP density.  The call has its own workspace, allocated and freed per call, and
// reads nothing of the handle's state but the genotypes and the list of kept rows: k_roh_mark writes the in-ROH bit of every
// (row, sample), k_roh_runs counts the reported runs of every row split and k_roh_stitch joins those that cross a split boundary, the
// stitch's scan over the splits and a scan over the samples on the host give every (sample, split) its place, and the fill pass of
// the same two kernels writes the records there.
#include "gpca_internal.h"

using namespace gpca;

namespace {
struct RohWs {
    uint8_t *plane = nullptr, *brk = nullptr;
    int* dom = nullptr;
    unsigned *cnt = nullptr, *rec = nullptr, *seg_count = nullptr, *segs = nullptr;
    unsigned long long *base = nullptr, *bad = nullptr;
    ~RohWs() { dfree(plane); dfree(brk); dfree(dom); dfree(cnt); dfree(rec); dfree(seg_count); dfree(segs); dfree(base); dfree(bad); }
};
}  // namespace

extern "C" int gpca_roh(gpca_handle* h, int64_t row0, int64_t row1, const uint8_t* brk, const gpca_roh_params* params, uint32_t* seg_count,
                        uint32_t* segs, int64_t cap, int64_t* n_found) {
    if (!h) return GPCA_ERR_BAD_ARG;
    LOCK(h);
    static const std::string f("gpca_roh");
    if (!have_genotypes(h)) return fail(h, GPCA_ERR_STATE, f + ": no genotypes resident");
    if (h->sm.on) return fail(h, GPCA_ERR_STATE, f + ": the handle streams its matrix in panels, which is not implemented");
    if (multi_rank(h)) return fail(h, GPCA_ERR_STATE, f + ": the handle holds a shard of the rows, which is not implemented");
    if (!h->have_stats) return fail(h, GPCA_ERR_STATE, f + ": no standardisation: run gpca_snp_stats or gpca_set_standardization first");
    if (h->n_pca == 0) return fail(h, GPCA_ERR_STATE, f + ": no kept row (the keep mask is empty)");
    const int64_t K = h->n_pca, N = h->N;
    if (!params) return fail(h, GPCA_ERR_BAD_ARG, f + ": params is required");
    if (!seg_count || !n_found) return fail(h, GPCA_ERR_BAD_ARG, f + ": seg_count and n_found are required");
    if (cap < 0 || ((segs == nullptr) != (cap == 0)))
        return fail(h, GPCA_ERR_BAD_ARG, f + ": segs holds cap >= 0 records and is NULL iff cap = 0");
    if (row0 < 0 || row1 < row0 || row1 > K)
        return fail(h, GPCA_ERR_BAD_ARG, f + ": rows must satisfy 0 <= row0 <= row1 <= K (K = " + std::to_string(K) + " kept rows)");
    const int64_t rows = row1 - row0;
    if (rows >= ((int64_t)1 << 31)) return fail(h, GPCA_ERR_BAD_ARG, f + ": a band of 2^31 or more rows (the row indices are 32-bit): ask for fewer rows");
    if (K >= ((int64_t)1 << 32) || N >= ((int64_t)1 << 32)) return fail(h, GPCA_ERR_BAD_ARG, f + ": 2^32 or more kept rows or samples (a record holds 32-bit indices)");
    const gpca_roh_params& p = *params;
    if (p.window_snp < 1 || p.window_snp > GPCA_ROH_WINDOW_MAX)
        return fail(h, GPCA_ERR_BAD_ARG, f + ": window_snp = " + std::to_string(p.window_snp) + " is outside 1 .. " + std::to_string(GPCA_ROH_WINDOW_MAX));
    if (p.window_het < 0 || p.window_het > p.window_snp || p.window_missing < 0 || p.window_missing > p.window_snp)
        return fail(h, GPCA_ERR_BAD_ARG, f + ": window_het and window_missing must lie in 0 .. window_snp");
    if (p.thr_den < 1 || p.thr_den > kRohMaxDen || p.thr_num < 0 || p.thr_num > p.thr_den)
        return fail(h, GPCA_ERR_BAD_ARG, f + ": the threshold needs 0 <= thr_num <= thr_den and 1 <= thr_den <= 2^20");
    if (p.min_snp < 1) return fail(h, GPCA_ERR_BAD_ARG, f + ": min_snp must be at least 1");
    if (p.max_het < -1) return fail(h, GPCA_ERR_BAD_ARG, f + ": max_het must be -1 (no limit) or at least 0");
    if (rows > 0 && !brk) return fail(h, GPCA_ERR_BAD_ARG, f + ": brk is required");
    // the break bytes as the kernels take them (row 0 of the band starts a domain), and the domains' first rows
    std::vector<uint8_t> hb((size_t)rows);
    std::vector<int> dom;
    for (int64_t j = 0; j < rows; ++j) {
        const uint8_t b = j == 0 ? (uint8_t)3 : brk[j];
        if ((b & ~3u) != 0u || b == 1u)
            return fail(h, GPCA_ERR_BAD_ARG, f + ": brk[" + std::to_string(j) + "] = " + std::to_string((int)b) +
                                                 " (bit 0 = a domain starts, bit 1 = no run continues into the row; bit 0 needs bit 1)");
        hb[(size_t)j] = b;
        if (b & 1u) dom.push_back((int)j);
    }
    std::fill(seg_count, seg_count + N, 0u);
    *n_found = 0;
    if (rows == 0) return GPCA_OK;
    const int64_t domains = (int64_t)dom.size();
    dom.push_back((int)rows);
    HIPCHK(hipSetDevice(h->device));
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
    int64_t forced = 0;
    if (const char* e = std::getenv("GPCA_ROH_SPLITS")) {                            // read per call: the tests' way to every split edge
        forced = std::strtoll(e, nullptr, 10);
        if (forced < 1) forced = 1;
    }
    const RohPlan plan = roh_plan(rows, N, cus, forced);
    if (sc_grid(plan) >= ((int64_t)1 << 31)) return fail(h, GPCA_ERR_BAD_ARG, f + ": the band makes 2^31 or more workgroups: ask for fewer rows");
    HIPCHK(hipStreamSynchronize(h->st));
    CHK(preflight_device_memory(h, f.c_str(), "the band needs", roh_call_bytes(N, rows, plan.splits, domains, 0) + (double)(64 << 20)));
    const bool packed = h->storage == GPCA_STORE_2BIT;
    const auto [G, ldr] = panel_rows(h, resident_view(h));
    hipStream_t st = h->st;
    RohWs ws;
    HIPCHK(dalloc(ws.plane, (size_t)roh_plane_capacity(rows, N))); HIPCHK(dalloc(ws.brk, (size_t)roh_brk_capacity(rows)));
    HIPCHK(dalloc(ws.dom, (size_t)roh_dom_capacity(domains))); HIPCHK(dalloc(ws.cnt, (size_t)roh_cnt_capacity(plan.splits, N)));
    HIPCHK(dalloc(ws.rec, (size_t)roh_rec_capacity(plan.splits, N)));
    HIPCHK(dalloc(ws.seg_count, (size_t)roh_segcount_capacity(N))); HIPCHK(dalloc(ws.base, (size_t)roh_base_capacity(N)));
    HIPCHK(dalloc(ws.bad, 1));
    HIPCHK(hipMemcpyAsync(ws.brk, hb.data(), (size_t)rows, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ws.dom, dom.data(), (size_t)roh_dom_capacity(domains) * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(ws.bad, 0xff, 8, st));
    // bytes as DESIGN counts them: the band's calls twice (entering and leaving the window) and once more under runs, the plane once
    // written and twice read
    const double band_bytes = (double)rows * (double)N * (packed ? 0.25 : 1.0), plane_bytes = (double)roh_plane_capacity(rows, N);
    {
        // "roh" = the call's device time up to the counts; "roh_mark" and "roh_count" inside it are its two passes over the band
        ScopedTimer t(h, "roh", 2.0 * (double)rows * (double)N, 3.0 * band_bytes + 2.0 * plane_bytes);
        {
            ScopedTimer tm(h, "roh_mark", (double)rows * (double)N, 2.0 * band_bytes + plane_bytes);
            if (launch_roh_mark(st, G, packed, ldr, h->d_pca_rows, N, row0, row1, plan, ws.dom, domains, p.window_snp, p.window_het,
                                p.window_missing, p.thr_num, p.thr_den, ws.plane, ws.bad) != 0)
                return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
            HIPCHK(hipGetLastError());
        }
        {
            ScopedTimer tc(h, "roh_count", (double)rows * (double)N, band_bytes + plane_bytes);
            if (launch_roh_runs(st, G, packed, ldr, h->d_pca_rows, N, row0, row1, plan, ws.brk, ws.plane, p.min_snp, p.max_het, ws.rec, ws.cnt, ws.seg_count, nullptr, nullptr, 0) != 0)
                return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
            HIPCHK(hipGetLastError());
        }
    }
    CHK(asc_check_genotypes(h, f, ws.bad, st));
    HIPCHK(hipMemcpyAsync(seg_count, ws.seg_count, (size_t)N * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<unsigned long long> base((size_t)N);
    unsigned long long total = 0;
    for (int64_t n = 0; n < N; ++n) { base[(size_t)n] = total; total += seg_count[n]; }
    *n_found = (int64_t)total;
    const int64_t records = std::min<int64_t>(cap, (int64_t)total);
    if (records == 0) return GPCA_OK;
    CHK(preflight_device_memory(h, f.c_str(), "the records need", 4.0 * (double)roh_seg_capacity(records) + (double)(64 << 20)));
    HIPCHK(dalloc(ws.segs, (size_t)roh_seg_capacity(records)));
    HIPCHK(hipMemcpyAsync(ws.base, base.data(), (size_t)N * 8, hipMemcpyHostToDevice, st));
    {
        ScopedTimer t(h, "roh_fill", (double)rows * (double)N, band_bytes + plane_bytes);
        if (launch_roh_runs(st, G, packed, ldr, h->d_pca_rows, N, row0, row1, plan, ws.brk, ws.plane, p.min_snp, p.max_het, ws.rec, ws.cnt, nullptr, ws.base, ws.segs, records) != 0)
            return fail(h, GPCA_ERR_BAD_ARG, f + ": the launch was refused");
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(segs, ws.segs, (size_t)roh_seg_capacity(records) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GPCA_OK;
}

extern "C" int gpca_roh_select(const uint32_t* segs, int64_t n, const int64_t* pos, int64_t min_bp, int64_t max_bp_per_snp, uint8_t* keep) {
    if (n < 0 || min_bp < 0 || max_bp_per_snp < 0 || (n > 0 && (!segs || !pos || !keep))) return GPCA_ERR_BAD_ARG;
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t first = segs[5 * i + 1], last = segs[5 * i + 2];
        if (last < first) return GPCA_ERR_BAD_ARG;
        const int64_t span = pos[last] - pos[first], nsnp = (int64_t)last - (int64_t)first + 1;
        // span <= max_bp_per_snp nsnp as ceil(span / nsnp) <= max_bp_per_snp: the product could pass 2^63
        keep[i] = (span >= min_bp && span / nsnp + (span % nsnp != 0 ? 1 : 0) <= max_bp_per_snp) ? 1 : 0;
    }
    return GPCA_OK;
}
