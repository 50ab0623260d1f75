// gpca_king (include/gpca.h section a9): KING-robust kinship of every pair of one row band of the strictly lower triangle, from the
// handle's kept rows.  One sweep over the resident matrix or the streamed panels (king.hip); the call has its own workspace, allocated
// and freed per call, and reads nothing of the handle's state but the keep mask of its standardisation.
#include "gpca_internal.h"

using namespace gpca;

namespace {
struct KingWs {
    double* kin = nullptr;
    int* counts = nullptr;
    uint32_t* kmask = nullptr;
    uint8_t* keep = nullptr;
    int2* tiles = nullptr;
    unsigned *het = nullptr, *miss = nullptr, *bad = nullptr;    // (device memory: the per-sample counts take atomics)
    ~KingWs() { dfree(kin); dfree(counts); dfree(kmask); dfree(keep); dfree(tiles); dfree(het); dfree(miss); dfree(bad); }
};
}  // namespace

extern "C" int gpca_king(gpca_handle* h, int64_t row0, int64_t row1, double* kinship, int32_t* counts) {
    if (!h) return GPCA_ERR_BAD_ARG;
    if (!kinship) return fail(h, GPCA_ERR_BAD_ARG, "gpca_king: kinship is required");
    LOCK(h);
    if (!have_genotypes(h)) return fail(h, GPCA_ERR_STATE, "gpca_king: no genotypes resident and no panel stream open");
    const int64_t M = h->M, N = h->N, Mpad = h->Mpad, Npad = h->ldg;
    if (row0 < 0 || row1 <= row0 || row1 > N)
        return fail(h, GPCA_ERR_BAD_ARG, "gpca_king: rows must satisfy 0 <= row0 < row1 <= N (N = " + std::to_string(N) + ")");
    if (!h->have_stats) return fail(h, GPCA_ERR_STATE, "gpca_king: no standardisation: run gpca_snp_stats or gpca_set_standardization first");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->st));
    const bool mr = multi_rank(h);
    const bool packed = h->storage == GPCA_STORE_2BIT;
    const int64_t E = band_entries(row0, row1, false);                    // strictly lower: row j holds j entries
    int lrc = GPCA_OK;                       // (the LOCAL rule: gpca_internal.h)

    // 1. the kept rows: their bit mask per 32-row block and their count
    std::vector<uint8_t> keep((size_t)M);
    HIPCHK(hipMemcpy(keep.data(), h->d_keep, (size_t)M, hipMemcpyDeviceToHost));
    std::vector<uint32_t> kmask;
    const int64_t K_local = kept_row_mask(keep, Mpad, kmask);
    constexpr int64_t kMaxK = (int64_t)1 << 31;
    if (!mr && K_local == 0) return fail(h, GPCA_ERR_STATE, "gpca_king: no kept row (the keep mask is empty)");
    if (K_local >= kMaxK) LOCAL(fail(h, GPCA_ERR_BAD_ARG, "gpca_king: 2^31 or more kept rows (the counts are 32-bit)"));

    // 2. preflight: everything the call allocates on the device, before any allocation
    const int64_t ntiles = band_tile_count(row0, row1, kKingTile);
    const size_t outn = (size_t)E * 5 + 2 * (size_t)Npad + 1 + 16;     // XX HH HM MH MM | het | miss | K | status slots: one exchange
    const double need = 8.0 * (double)outn + (counts ? 20.0 : 8.0) * (double)E + 8.0 * (double)Npad + (double)(Mpad / 32) * 4 + (double)M + 8.0 * (double)ntiles +
                        (64 << 20);
    LOCAL(preflight_device_memory(h, "gpca_king", "the band needs", need));

    KingWs ws;
    XBuf xb;
    HIPCHK(xb.alloc(outn));
    HIPCHK(hipMemsetAsync(xb.p, 0, outn * 8, h->st));
    double* const R = xb.p;
    double* const het = R + 5 * (size_t)E;
    double* const miss = het + Npad;
    std::vector<int2> tiles;
    auto prep = [&]() -> int {
        band_tile_list(row0, row1, kKingTile, tiles);
        HIPCHK(dalloc(ws.kmask, kmask.size())); HIPCHK(dalloc(ws.keep, M)); HIPCHK(dalloc(ws.tiles, tiles.size())); HIPCHK(dalloc(ws.bad, 1));
        HIPCHK(dalloc(ws.het, Npad)); HIPCHK(dalloc(ws.miss, Npad));
        HIPCHK(dalloc(ws.kin, E));
        if (counts) HIPCHK(dalloc(ws.counts, 3 * (size_t)E));
        hipStream_t st = h->st;
        HIPCHK(hipMemcpyAsync(ws.kmask, kmask.data(), kmask.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ws.keep, keep.data(), (size_t)M, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ws.tiles, tiles.data(), tiles.size() * sizeof(int2), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(ws.bad, 0, 4, st));
        HIPCHK(hipMemsetAsync(ws.het, 0, (size_t)Npad * 4, st)); HIPCHK(hipMemsetAsync(ws.miss, 0, (size_t)Npad * 4, st));
        HIPCHK(hipStreamSynchronize(st));
        return GPCA_OK;
    };
    LOCAL(prep());

    // 3. one sweep: per panel (or the resident matrix) the per-sample counts and the dosage check, then the triangle's tiles of the band
    auto sweep = [&]() -> int {
        const double elems = (double)M * (double)N;
        ScopedTimer t(h, "king", 2.0 * 2.0 * 32768.0 * (double)(Mpad / 32) * 16.0 * (double)ntiles, (packed ? elems / 4 : elems));
        CHK(for_each_panel(h, [&](const PanelView& pv) -> int {
            const auto [G, ldr] = panel_rows(h, pv);
            launch_king_vec(h->st, G, packed, ldr, pv.rows, Npad, ws.keep + pv.row0, ws.het, ws.miss, ws.bad);
            launch_king(h->st, G, packed, ldr, pv.rows_pad, ws.kmask + (pv.row0 >> 5), ws.tiles, ntiles, row0, row1, N, R, E,
                        pv.index == 0 ? 1 : 0);
            HIPCHK(hipGetLastError());
            return GPCA_OK;
        }));
        launch_king_vec_f64(h->st, ws.het, ws.miss, Npad, het, miss);
        HIPCHK(hipGetLastError());
        return GPCA_OK;
    };
    LOCAL(sweep());
    LOCAL(check_genotype_flag(h, "gpca_king", "kept", ws.bad));

    // 4. sharded handles: one exchange of the integer counts (exact in f64 below 2^53), the kept-row count and the status word; the
    //    kinship is computed after the sum, so every rank gets the one-rank bits
    double K_total = (double)K_local;
    if (mr) {
        double* slot = xb.p + outn - 17;
        const double kl = lrc == GPCA_OK ? (double)K_local : 0.0;
        // (kl is a stack variable: the stream is synchronised before it goes out of use; gpca_grm's exchanges carry no such value)
        if ((hipMemcpyAsync(slot, &kl, 8, hipMemcpyHostToDevice, h->st) != hipSuccess || hipStreamSynchronize(h->st) != hipSuccess) && lrc == GPCA_OK)
            lrc = fail(h, GPCA_ERR_HIP, "gpca_king: status copy failed");
        double slots[17];
        CHK(exchange_with_status(h, "gpca_king", xb.p, outn, lrc, slots, 17));
        if (lrc != GPCA_OK) return lrc;
        K_total = slots[0];
        if (K_total < 0.5) return fail(h, GPCA_ERR_STATE, "gpca_king: no kept row on any rank (the keep masks are empty)");
        if (K_total >= (double)kMaxK) return fail(h, GPCA_ERR_BAD_ARG, "gpca_king: 2^31 or more kept rows over the ranks (the counts are 32-bit)");
    }
    if (lrc != GPCA_OK) return lrc;

    // 5. the kinship of the band from the summed counts
    launch_king_finish(h->st, R, E, het, miss, K_total, row0, row1, ws.kin, ws.counts);
    HIPCHK(hipGetLastError());
    if (E > 0) {
        HIPCHK(hipMemcpyAsync(kinship, ws.kin, (size_t)E * 8, hipMemcpyDeviceToHost, h->st));
        if (counts) HIPCHK(hipMemcpyAsync(counts, ws.counts, (size_t)E * 12, hipMemcpyDeviceToHost, h->st));
    }
    HIPCHK(hipStreamSynchronize(h->st));
    return GPCA_OK;
}
