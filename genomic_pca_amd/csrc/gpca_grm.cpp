// gpca_grm (include/gpca.h section a8): the genetic relationship matrix of the handle's kept rows, one row band of its lower triangle.
// One sweep over the resident matrix or the streamed panels (grm.hip); the call has its own workspace, allocated and freed per call, and
// reads nothing of the handle's fitted state but the standardisation.
#include "gpca_internal.h"

using namespace gpca;

namespace {
struct GrmWs {
    double *R = nullptr, *Up = nullptr, *Vp = nullptr, *u = nullptr, *v = nullptr;
    int* Q = nullptr;
    int8_t* tab = nullptr;
    uint32_t* kmask = nullptr;
    int64_t *qc = nullptr, *qe = nullptr;
    uint8_t* keep = nullptr;
    int2* tiles = nullptr;
    unsigned *cnt = nullptr, *bad = nullptr;
    ~GrmWs() {
        dfree(R); dfree(Up); dfree(Vp); dfree(u); dfree(v); dfree(Q); dfree(tab); dfree(kmask); dfree(qc); dfree(qe); dfree(keep);
        dfree(tiles); dfree(cnt); dfree(bad);
    }
};
constexpr double kGrmQMax = 4398046511103.0;   // 128^kGrmDigits - 1
static_assert(kGrmDigits == 6, "kGrmQMax");
}  // namespace

extern "C" int gpca_grm(gpca_handle* h, int32_t scaling, int64_t row0, int64_t row1, double* grm, float* npairs) {
    if (!h) return GPCA_ERR_BAD_ARG;
    if (!grm) return fail(h, GPCA_ERR_BAD_ARG, "gpca_grm: grm is required");
    if (scaling != GPCA_GRM_STANDARDIZED && scaling != GPCA_GRM_CENTRED)
        return fail(h, GPCA_ERR_BAD_ARG, "gpca_grm: scaling must be GPCA_GRM_STANDARDIZED or GPCA_GRM_CENTRED");
    LOCK(h);
    if (!have_genotypes(h)) return fail(h, GPCA_ERR_STATE, "gpca_grm: no genotypes resident and no panel stream open");
    const int64_t M = h->M, N = h->N, Mpad = h->Mpad, Npad = h->ldg;
    if (row0 < 0 || row1 <= row0 || row1 > N)
        return fail(h, GPCA_ERR_BAD_ARG, "gpca_grm: rows must satisfy 0 <= row0 < row1 <= N (N = " + std::to_string(N) + ")");
    if (!h->have_stats) return fail(h, GPCA_ERR_STATE, "gpca_grm: no standardisation: run gpca_snp_stats or gpca_set_standardization first");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->st));
    const bool mr = multi_rank(h);
    const bool packed = h->storage == GPCA_STORE_2BIT;
    const int64_t E = band_entries(row0, row1, true);
    int lrc = GPCA_OK;                       // (the LOCAL rule: gpca_internal.h)

    // 1. the rows' values on the host: w = r^2, c = -r b, e = b^2 (centred: r = 1, b = -mu) of the kept rows, and their largest value
    std::vector<float> mu((size_t)M), r((size_t)M), b((size_t)M);
    std::vector<uint8_t> keep((size_t)M);
    HIPCHK(hipMemcpy(mu.data(), h->d_mu, (size_t)M * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(r.data(), h->d_r, (size_t)M * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(b.data(), h->d_b, (size_t)M * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(keep.data(), h->d_keep, (size_t)M, hipMemcpyDeviceToHost));
    std::vector<double> vw((size_t)M, 0.0), vc((size_t)M, 0.0), ve((size_t)M, 0.0);
    std::vector<uint32_t> kmask;
    const int64_t K_local = kept_row_mask(keep, Mpad, kmask);
    double vmax = 0.0;
    auto scan = [&]() -> int {
        for (int64_t i = 0; i < M; ++i) {
            if (!keep[(size_t)i]) continue;
            const double ri = scaling == GPCA_GRM_CENTRED ? 1.0 : (double)r[(size_t)i];
            const double bi = scaling == GPCA_GRM_CENTRED ? -(double)mu[(size_t)i] : (double)b[(size_t)i];
            const double w = ri * ri, c = -ri * bi, e = bi * bi;
            if (!std::isfinite(w) || !std::isfinite(c) || !std::isfinite(e) || c < 0.0)
                return fail(h, GPCA_ERR_BAD_ARG, "gpca_grm: kept row " + std::to_string(i + h->snp_offset) +
                                                     " has a non-finite or negative mean, or a non-finite scale");
            vw[(size_t)i] = w; vc[(size_t)i] = c; ve[(size_t)i] = e;
            vmax = std::max(vmax, std::max(2.0 * w, std::max(c, e)));
        }
        return GPCA_OK;
    };
    LOCAL(scan());

    // 2. preflight: everything the call allocates on the device, before any allocation
    const int64_t rows_max = h->sm.on ? std::min<int64_t>(h->sm.panel_rows, M) : M;
    const int64_t ngroups = (rows_max + kGrmFlushRows - 1) / kGrmFlushRows;
    const int64_t ntiles = band_tile_count(row0, row1, kGrmTile);
    const size_t outn = (size_t)E * (npairs ? 2 : 1) + 16;           // band | npairs | status slots: one exchange
    const double need = 12.0 * (double)E + 8.0 * (double)outn + (double)(Mpad / 32) * (kGrmTabBytes + 4) + 17.0 * (double)M +
                        16.0 * (double)ngroups * (double)Npad + 20.0 * (double)Npad + 8.0 * (double)ntiles + (64 << 20);
    LOCAL(preflight_device_memory(h, "gpca_grm", "the band needs", need));

    // 3. sharded handles: one small exchange of every rank's largest value, kept-row count and status, so that every rank quantises on
    //    the scale one rank would use (the integer sums stay the one-rank ones) and a failure so far reaches every rank
    double K_total = (double)K_local;
    if (mr) {
        const size_t xn = (size_t)h->world + 1 + 16;
        XBuf xb;
        std::vector<double> hx(xn, 0.0);
        auto body = [&]() -> int {
            HIPCHK(xb.alloc(xn));
            if (lrc == GPCA_OK) { hx[(size_t)h->rank] = vmax; hx[(size_t)h->world] = (double)K_local; }
            HIPCHK(hipMemcpyAsync(xb.p, hx.data(), xn * 8, hipMemcpyHostToDevice, h->st));
            return exchange_with_status(h, "gpca_grm", xb.p, xn, lrc, hx.data(), xn);
        };
        CHK(body());
        if (lrc != GPCA_OK) return lrc;
        vmax = 0.0;
        for (int k = 0; k < h->world; ++k) vmax = std::max(vmax, hx[(size_t)k]);
        K_total = hx[(size_t)h->world];
    }
    if (K_total < 0.5) return fail(h, GPCA_ERR_STATE, "gpca_grm: no kept row (the keep mask is empty)");

    // 4. the common scale S = 2^s (the smallest power of two with vmax / S <= 128^6 - 1) and the digit tables
    double S = 1.0;
    if (vmax > 0.0) {
        int ex = 0;
        (void)std::frexp(vmax / kGrmQMax, &ex);
        S = std::ldexp(1.0, ex);
        while (vmax / (S * 0.5) <= kGrmQMax) S *= 0.5;
        while (vmax / S > kGrmQMax) S *= 2.0;
    }
    std::vector<int8_t> tab((size_t)(Mpad / 32) * kGrmTabBytes, 0);
    std::vector<int64_t> qc((size_t)M, 0), qe((size_t)M, 0);
    unsigned __int128 qe_sum = 0;
    for (int64_t i = 0; i < M; ++i) {
        if (!keep[(size_t)i]) continue;
        const int64_t q[4] = {(int64_t)std::llround(vw[(size_t)i] / S), (int64_t)std::llround(2.0 * vw[(size_t)i] / S),
                              (int64_t)std::llround(vc[(size_t)i] / S), (int64_t)std::llround(ve[(size_t)i] / S)};
        int8_t* tb = tab.data() + (size_t)(i >> 5) * kGrmTabBytes + (i & 31);
        for (int t = 0; t < 4; ++t)
            for (int d = 0; d < kGrmDigits; ++d) tb[(t * kGrmDigits + d) * 32] = (int8_t)((q[t] >> (7 * d)) & 127);
        qc[(size_t)i] = q[2]; qe[(size_t)i] = q[3]; qe_sum += (unsigned __int128)q[3];
    }
    const double beta = (double)qe_sum;

    GrmWs ws;
    XBuf xout;
    HIPCHK(xout.alloc(outn));
    double* const out = xout.p;
    HIPCHK(hipMemsetAsync(out, 0, outn * 8, h->st));
    std::vector<int2> tiles;
    band_tile_list(row0, row1, kGrmTile, tiles);
    auto prep = [&]() -> int {
        HIPCHK(dalloc(ws.R, E)); HIPCHK(dalloc(ws.Q, E));
        HIPCHK(dalloc(ws.tab, tab.size())); HIPCHK(dalloc(ws.kmask, kmask.size()));
        HIPCHK(dalloc(ws.qc, M)); HIPCHK(dalloc(ws.qe, M)); HIPCHK(dalloc(ws.keep, M));
        HIPCHK(dalloc(ws.Up, (size_t)ngroups * Npad)); HIPCHK(dalloc(ws.Vp, (size_t)ngroups * Npad));
        HIPCHK(dalloc(ws.u, Npad)); HIPCHK(dalloc(ws.v, Npad)); HIPCHK(dalloc(ws.cnt, Npad)); HIPCHK(dalloc(ws.bad, 1));
        HIPCHK(dalloc(ws.tiles, tiles.size()));
        hipStream_t st = h->st;
        HIPCHK(hipMemcpyAsync(ws.tab, tab.data(), tab.size(), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ws.kmask, kmask.data(), kmask.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ws.qc, qc.data(), (size_t)M * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ws.qe, qe.data(), (size_t)M * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ws.keep, keep.data(), (size_t)M, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ws.tiles, tiles.data(), tiles.size() * sizeof(int2), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(ws.u, 0, (size_t)Npad * 8, st)); HIPCHK(hipMemsetAsync(ws.v, 0, (size_t)Npad * 8, st));
        HIPCHK(hipMemsetAsync(ws.cnt, 0, (size_t)Npad * 4, st)); HIPCHK(hipMemsetAsync(ws.bad, 0, 4, st));
        HIPCHK(hipStreamSynchronize(st));    // (the host tables go out of scope only at the end, but keep the copies simple)
        return GPCA_OK;
    };
    LOCAL(prep());

    // 5. one sweep: per panel (or the resident matrix) the vectors and the dosage check, then the triangle's tiles of the band
    auto sweep = [&]() -> int {
        const double elems = (double)M * (double)N;
        ScopedTimer t(h, "grm", 2.0 * kGrmDigits * (double)M * 4096.0 * (double)ntiles, (packed ? elems / 4 : elems));
        CHK(for_each_panel(h, [&](const PanelView& pv) -> int {
            const auto [G, ldr] = panel_rows(h, pv);
            const size_t blk0 = (size_t)(pv.row0 >> 5);
            launch_grm_vec(h->st, G, packed, ldr, pv.rows, Npad, ws.keep + pv.row0, ws.qc + pv.row0, ws.qe + pv.row0, ws.Up, ws.Vp, ws.cnt, ws.bad);
            launch_grm_vec_fold(h->st, ws.Up, ws.Vp, pv.rows, Npad, ws.u, ws.v);
            launch_grm(h->st, G, packed, ldr, pv.rows_pad, ws.tab + blk0 * kGrmTabBytes, ws.kmask + blk0, ws.tiles, ntiles, row0, row1, N,
                       ws.R, ws.Q, pv.index == 0 ? 1 : 0);
            HIPCHK(hipGetLastError());
            return GPCA_OK;
        }));
        launch_grm_finish(h->st, ws.R, ws.Q, ws.u, ws.v, ws.cnt, S, beta, (double)K_local, row0, row1, out, npairs ? out + E : nullptr);
        HIPCHK(hipGetLastError());
        return GPCA_OK;
    };
    LOCAL(sweep());
    LOCAL(check_genotype_flag(h, "gpca_grm", "kept", ws.bad));

    // 6. sharded handles: one exchange of band, counts and status word (the numerators and NPAIRS are sums over the ranks' rows)
    if (mr) {
        double slots[16];
        CHK(exchange_with_status(h, "gpca_grm", out, outn, lrc, slots));
    }
    if (lrc != GPCA_OK) return lrc;
    HIPCHK(hipMemcpyAsync(grm, out, (size_t)E * 8, hipMemcpyDeviceToHost, h->st));
    std::vector<double> np(npairs ? (size_t)E : 0);
    if (npairs) HIPCHK(hipMemcpyAsync(np.data(), out + E, (size_t)E * 8, hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
    for (int64_t i = 0; i < E; ++i) grm[i] /= K_total;
    if (npairs) for (int64_t i = 0; i < E; ++i) npairs[i] = (float)np[(size_t)i];
    return GPCA_OK;
}
