// gpca_project (include/gpca.h section a7): the handle's genotypes projected onto a caller's model (mu, sigma, W), missing calls
// mean-imputed.  One sweep over the resident matrix or the streamed panels (project.hip); nothing of the handle's fitted state is read
// or written -- the call has its own workspace, allocated and freed per call.
#include "gpca_internal.h"

using namespace gpca;

// default of the LAZYB choice of k_project (DESIGN.md section 7 has the measurement behind it)
constexpr int kProjectLazyB = 0;

namespace {
// device workspace of one call (freed on every exit path)
struct ProjWs {
    float *mu = nullptr, *sigma = nullptr, *r = nullptr, *b = nullptr, *Wa = nullptr, *Wb = nullptr, *cpart = nullptr, *cpart_b = nullptr;
    uint8_t* keep = nullptr;
    uint32_t* rmask = nullptr;
    int8_t *Ta = nullptr, *Tb = nullptr;
    double *c = nullptr, *scratch = nullptr, *part = nullptr, *tsa = nullptr, *tia = nullptr, *tsb = nullptr, *tib = nullptr;
    double *Ypa = nullptr, *Ypb = nullptr, *Yia = nullptr, *Yib = nullptr;
    unsigned *cnt = nullptr, *bad = nullptr;
    ~ProjWs() {
        dfree(mu); dfree(sigma); dfree(r); dfree(b); dfree(Wa); dfree(Wb); dfree(cpart); dfree(cpart_b); dfree(keep); dfree(rmask);
        dfree(Ta); dfree(Tb); dfree(c); dfree(scratch); dfree(part); dfree(tsa); dfree(tia); dfree(tsb); dfree(tib);
        dfree(Ypa); dfree(Ypb); dfree(Yia); dfree(Yib); dfree(cnt); dfree(bad);
    }
};
}  // namespace

extern "C" int gpca_project(gpca_handle* h, const float* mu, const float* sigma, const float* W, int32_t k, double* scores, int32_t* n_used) {
    if (!h) return GPCA_ERR_BAD_ARG;
    if (!mu || !sigma || !W || !scores) return fail(h, GPCA_ERR_BAD_ARG, "gpca_project: mu, sigma, W and scores are required");
    if (k < 1 || k > kMaxSketch) return fail(h, GPCA_ERR_BAD_ARG, "gpca_project: k must be in [1, 128]");
    LOCK(h);
    if (!have_genotypes(h)) return fail(h, GPCA_ERR_STATE, "gpca_project: no genotypes resident and no panel stream open");
    if (h->precision != GPCA_PREC_I8_EXACT) return fail(h, GPCA_ERR_STATE, "gpca_project: needs the exact-integer precision (GPCA_PREC_I8_EXACT)");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->st));
    const bool mr = multi_rank(h);
    const int64_t M = h->M, N = h->N, Mpad = h->Mpad, Npad = h->ldg;
    const int Lp = (int)round_up(k, 32), halves = Lp / 32;
    int lrc = GPCA_OK;                       // (the LOCAL rule: gpca_internal.h)

    // 1. the model on the host: rows with a nonzero W row are in it; those need finite mu, sigma, W and sigma > 0
    std::vector<uint8_t> keep((size_t)M, 0);
    std::vector<uint32_t> rmask((size_t)(Mpad / 32), 0u);
    std::vector<float> Wp((size_t)Mpad * Lp, 0.f);
    int64_t n_model = 0;
    auto scan = [&]() -> int {
        for (int64_t i = 0; i < M; ++i) {
            const float* wi = W + (size_t)i * k;
            bool in = false, finite = true;
            for (int c = 0; c < k; ++c) { in |= wi[c] != 0.f; finite &= std::isfinite(wi[c]); }
            if (!in) continue;
            if (!finite || !std::isfinite(mu[i]) || !std::isfinite(sigma[i]) || !(sigma[i] > 0.f))
                return fail(h, GPCA_ERR_BAD_ARG, "gpca_project: model row " + std::to_string(i + h->snp_offset) +
                                                     " has a non-finite mu, sigma or W entry, or sigma <= 0");
            keep[(size_t)i] = 1; set_row_bit(rmask, i); ++n_model;
            std::copy(wi, wi + k, Wp.begin() + (size_t)i * Lp);
        }
        return GPCA_OK;
    };
    LOCAL(scan());

    ProjWs ws;
    const size_t outn = (size_t)N * Lp + (size_t)N + 16;            // scores | used | status slots: one exchange
    XBuf xout;                                                     // (first: a rank that fails below still has its block to exchange)
    HIPCHK(xout.alloc(outn));
    double* const out = xout.p;
    HIPCHK(hipMemsetAsync(out, 0, outn * 8, h->st));
    const bool packed = h->storage == GPCA_STORE_2BIT;
    // measurement knob: 1 = the indicator planes are loaded only for blocks that hold a missing code (project.hip, LAZYB)
    const char* lz = std::getenv("GPCA_PROJECT_LAZY_B");
    const int lazy_b = lz ? std::atoi(lz) : kProjectLazyB;
    const size_t td_half = (size_t)Mpad * 32 * kDigits;
    // the most row chunks any launch of the sweep will write partials for (a panel's plan is not monotone in its rows: ask each size)
    int64_t max_W = prj_plan(Mpad, Npad, h->gtt_waves_target).W;
    if (h->sm.on)
        for (int p = 0; p < h->sm.n_panels; p += std::max(1, h->sm.n_panels - 1)) {
            const int64_t rows = std::min(h->sm.panel_rows, M - (int64_t)p * h->sm.panel_rows);
            max_W = std::max<int64_t>(max_W, prj_plan(round_up(rows, kGQRowsPerWave), Npad, h->gtt_waves_target).W);
        }
    auto prep = [&]() -> int {
        HIPCHK(dalloc(ws.mu, M)); HIPCHK(dalloc(ws.sigma, M)); HIPCHK(dalloc(ws.keep, M));
        HIPCHK(dalloc(ws.r, Mpad)); HIPCHK(dalloc(ws.b, Mpad)); HIPCHK(dalloc(ws.rmask, Mpad / 32));
        HIPCHK(dalloc(ws.Wa, (size_t)Mpad * Lp)); HIPCHK(dalloc(ws.Wb, (size_t)Mpad * Lp));
        HIPCHK(dalloc(ws.cpart, (size_t)project_cpart_capacity(Mpad, Lp))); HIPCHK(dalloc(ws.cpart_b, (size_t)project_cpart_capacity(Mpad, Lp)));
        HIPCHK(dalloc(ws.Ta, td_half * halves)); HIPCHK(dalloc(ws.Tb, td_half * halves));
        HIPCHK(dalloc(ws.c, Lp)); HIPCHK(dalloc(ws.scratch, (size_t)project_scratch_capacity(Lp))); HIPCHK(dalloc(ws.part, (size_t)project_part_capacity(Mpad, Lp)));
        HIPCHK(dalloc(ws.tsa, Lp)); HIPCHK(dalloc(ws.tia, Lp)); HIPCHK(dalloc(ws.tsb, Lp)); HIPCHK(dalloc(ws.tib, Lp));
        HIPCHK(dalloc(ws.Ypa, (size_t)max_W * Npad * 32)); HIPCHK(dalloc(ws.Ypb, (size_t)max_W * Npad * 32));
        HIPCHK(dalloc(ws.Yia, (size_t)N * Lp)); HIPCHK(dalloc(ws.Yib, (size_t)N * Lp));
        HIPCHK(dalloc(ws.cnt, Npad)); HIPCHK(dalloc(ws.bad, 1));
        hipStream_t st = h->st;
        HIPCHK(hipMemcpyAsync(ws.mu, mu, (size_t)M * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ws.sigma, sigma, (size_t)M * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ws.keep, keep.data(), (size_t)M, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ws.rmask, rmask.data(), rmask.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ws.Wa, Wp.data(), Wp.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(ws.r, 0, (size_t)Mpad * 4, st)); HIPCHK(hipMemsetAsync(ws.b, 0, (size_t)Mpad * 4, st));
        HIPCHK(hipMemsetAsync(ws.cnt, 0, (size_t)Npad * 4, st)); HIPCHK(hipMemsetAsync(ws.bad, 0, 4, st));
        // r = 1 / sigma, b = -mu r on the model rows (the kernel gpca_set_standardization uses: the same f32 roundings as the QC pass)
        launch_set_scale(st, M, ws.mu, ws.sigma, ws.keep, ws.r, ws.b);
        HIPCHK(hipGetLastError());
        // side a: r o W and c = b^T W, exactly as gpca_transform prepares its loadings; side b: b o W (its c is not used)
        launch_scale_rows(st, ws.Wa, M, Mpad, Lp, ws.b, ws.b, ws.Wb, ws.cpart_b, 0);
        launch_scale_rows(st, ws.Wa, M, Mpad, Lp, ws.r, ws.b, ws.Wa, ws.cpart, 0);
        HIPCHK(hipGetLastError());
        launch_sum_partials_f32(st, ws.cpart, omega_num_parts(Mpad), Lp, ws.c, ws.scratch);
        HIPCHK(hipGetLastError());
        if (mr) return GPCA_OK;           // (the digit scales of a sharded model wait for the column maxima of every rank, below)
        for (int hf = 0; hf < halves; ++hf) {
            launch_quantize_f32(st, ws.Wa + 32 * hf, Mpad, Mpad, ws.part, ws.tsa + 32 * hf, ws.tia + 32 * hf, ws.Ta + hf * td_half, 0, h->nd, Lp);
            launch_quantize_f32(st, ws.Wb + 32 * hf, Mpad, Mpad, ws.part, ws.tsb + 32 * hf, ws.tib + 32 * hf, ws.Tb + hf * td_half, 0, h->nd, Lp);
        }
        HIPCHK(hipGetLastError());
        return GPCA_OK;
    };
    LOCAL(prep());
    // Row-sharded model: the digit planes of every rank use the column maxima of the WHOLE model (gathered through one small exchange:
    // each rank fills its own slot), so every row gets the digits it gets on one rank -- the integer sums stay exact and the ranks'
    // result is the unsharded one up to the f64 order of the final sums.  A rank that has failed contributes zeros and goes on to the
    // status exchange at the end.
    auto shard_scales = [&]() -> int {
        const size_t per = 2 * (size_t)Lp, xn = (size_t)h->world * per;
        XBuf xb;
        HIPCHK(xb.alloc(xn));
        double* const dx = xb.p;
        std::vector<double> hx(xn, 0.0);
        int rc = GPCA_OK;
        auto body = [&]() -> int {
            HIPCHK(hipMemsetAsync(dx, 0, xn * 8, h->st));
            if (lrc == GPCA_OK) {
                unsigned long long* mx = (unsigned long long*)(dx + (size_t)h->rank * per);
                launch_project_colmax(h->st, ws.Wa, Mpad, Lp, mx);
                launch_project_colmax(h->st, ws.Wb, Mpad, Lp, mx + Lp);
                HIPCHK(hipGetLastError());
            }
            CHK(allreduce_f64(h, dx, (int64_t)xn));
            HIPCHK(hipMemcpyAsync(hx.data(), dx, xn * 8, hipMemcpyDeviceToHost, h->st));
            HIPCHK(hipStreamSynchronize(h->st));
            return GPCA_OK;
        };
        rc = body();
        if (rc != GPCA_OK || lrc != GPCA_OK) return rc;
        std::vector<double> gmax(per, 0.0);
        for (int r = 0; r < h->world; ++r)
            for (size_t j = 0; j < per; ++j) gmax[j] = std::max(gmax[j], hx[(size_t)r * per + j]);
        HIPCHK(hipMemcpyAsync(ws.part, gmax.data(), per * 8, hipMemcpyHostToDevice, h->st));
        for (int hf = 0; hf < halves; ++hf) {
            launch_quantize_f32_premax(h->st, ws.Wa + 32 * hf, Mpad, Mpad, ws.part + 32 * hf, 1, ws.tsa + 32 * hf, ws.tia + 32 * hf, ws.Ta + hf * td_half, 0, h->nd, Lp);
            launch_quantize_f32_premax(h->st, ws.Wb + 32 * hf, Mpad, Mpad, ws.part + Lp + 32 * hf, 1, ws.tsb + 32 * hf, ws.tib + 32 * hf, ws.Tb + hf * td_half, 0, h->nd, Lp);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(h->st));     // (gmax is a host vector of this scope)
        return GPCA_OK;
    };
    if (mr) {
        const int src = shard_scales();
        if (src != GPCA_OK && lrc == GPCA_OK) lrc = src;
        if (src == GPCA_ERR_RCCL) return src;    // (the transport itself failed: no second exchange to meet at)
    }

    // 2. one sweep: every panel (or the resident matrix) read once per 32 columns; exact integer sums accumulated in f64 per half
    auto sweep = [&]() -> int {
        const double elems = (double)M * (double)N;
        ScopedTimer t(h, "project", 4.0 * elems * k, (packed ? elems / 4 : elems) * halves);
        CHK(for_each_panel(h, [&](const PanelView& pv) -> int {
            const PrjPlan plan = prj_plan(pv.rows_pad, Npad, h->gtt_waves_target);
            const auto [G, ldr] = panel_rows(h, pv);
            const size_t blk0 = (size_t)(pv.row0 >> 5);
            for (int hf = 0; hf < halves; ++hf) {
                launch_project(h->st, G, packed, ldr, pv.rows_pad, Npad, ws.Ta + hf * td_half + blk0 * kPlaneBytesPerBlock,
                               ws.Tb + hf * td_half + blk0 * kPlaneBytesPerBlock, ws.rmask + blk0, ws.Ypa, ws.Ypb, (hf == 0 ? ws.cnt : nullptr),
                               ws.bad, plan, h->nd, lazy_b);      // (the first half counts the missing calls)
                HIPCHK(hipGetLastError());
                const size_t yo = (size_t)hf * N * 32;
                launch_accum_y_i8(h->st, ws.Ypa, plan.W, Npad, N, ws.Yia + yo, pv.index == 0);
                launch_accum_y_i8(h->st, ws.Ypb, plan.W, Npad, N, ws.Yib + yo, pv.index == 0);
                HIPCHK(hipGetLastError());
            }
            return GPCA_OK;
        }));
        // scores = fma(tscale_a, S_a, c) (gpca_transform's combine), then the correction of the missing calls; used = n_model - missing
        for (int hf = 0; hf < halves; ++hf) {
            const size_t yo = (size_t)hf * N * 32;
            launch_finish_y_i8(h->st, ws.Yia + yo, N, ws.c + 32 * hf, ws.tsa + 32 * hf, out + 32 * hf, Lp);
            launch_project_correct(h->st, ws.Yib + yo, N, ws.tsb + 32 * hf, ws.cnt, n_model, out + 32 * hf, Lp);
        }
        launch_project_used(h->st, ws.cnt, N, (double)n_model, out + (size_t)N * Lp);
        HIPCHK(hipGetLastError());
        return GPCA_OK;
    };
    LOCAL(sweep());
    // the dosage check of the kernel: its verdict must be known before the exchange carries the status word
    LOCAL(check_genotype_flag(h, "gpca_project", "model", ws.bad));

    // 3. one exchange of scores, counts and the status word (sharded handles: exchange_with_status, the whole block comes back)
    std::vector<double> host(outn, 0.0);
    if (mr) CHK(exchange_with_status(h, "gpca_project", out, outn, lrc, host.data(), outn));
    else {
        HIPCHK(hipMemcpyAsync(host.data(), out, outn * 8, hipMemcpyDeviceToHost, h->st));
        HIPCHK(hipStreamSynchronize(h->st));
    }
    if (lrc != GPCA_OK) return lrc;
    for (int64_t n = 0; n < N; ++n) {
        for (int c = 0; c < k; ++c) scores[(size_t)n * k + c] = host[(size_t)n * Lp + c];
        if (n_used) n_used[n] = (int32_t)host[(size_t)N * Lp + n];
    }
    return GPCA_OK;
}
