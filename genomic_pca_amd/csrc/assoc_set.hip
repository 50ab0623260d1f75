// Gene-level set tests of the logistic score scan (gpca_assoc_logistic_set; gpca_assoc_score.cpp; include/gpca.h section a16): the
// covariance Phi = G~^T W G~ of the scores of the rows of one set, per trait, a weighted Gram over the sample axis.
//
// The score scan's count, main and finish kernels have run over the listed rows: sums (n_obs, s1, s2 and with them the flip) and
// dv (U, gwg and a_0 .. a_Pc per trait) exist for every listed row.  k_assoc_set_gram: a workgroup owns one (strip of 32 rows of a set's
// lower triangle, trait) and stages the set's rows [0, asg_staged_rows) exactly as k_assoc_score stages its tile (asc_fetch, asr_put:
// the operand x = g or 2 - g, the missing code for m, 0 outside S and past N; 64-sample stages, two LDS buffers, one barrier per stage),
// and beside them the stage's 64 values of w_t, the f32 panel column the score scan multiplies.  Wave v <= s owns the 32 x 32 tile
// (rows a of strip s, rows b of column block v).  Per 16-sample group, in the order (i, 8 + i) of assoc_tile.h:
//     XX += x_a (w x_b),     XM += x_a (w m_b)   (a missing call in the b rows),     MX += m_a (w x_b)   (one in the a rows),
//     MM += m_a (w m_b)   (both)
// The right-hand operands are w, 2 w or 0 and the left-hand ones 0, 1 or 2: every product of the v_mfma_f32_32x32x2_f32 is exact, and
// on the diagonal x_a (w x_a) = x_a^2 w is the product k_assoc_score adds to q in the same order, m_a (w m_a) the one it adds to e.  The
// four f32 accumulators go to f64 running sums every kAscFlush samples, counted from sample 0: XX_aa carries the bits of q and MM_aa
// those of e (a product of 0 more or less changes no sum).  No split of the sample axis and no atomics: an entry depends on its two
// rows, S, N and the trait alone.
// Epilogue (f64, no contraction): R_ab = (XX + (xbar_b XM + xbar_a MX)) + (xbar_a xbar_b) MM into Phi's packed lower triangle; then
// k_assoc_set_finish: Phi_ab = s_a s_b ((R_ab - a_a,0 a_b,0) - sum_{j = 1 .. Pc} a_a,j a_b,j), the sum formed first with j ascending,
// which on the diagonal is k_assoc_score_finish's V.
// Registers: 4 x 16 f32 accumulators and 4 x 16 f64 running sums per lane; the figures hipcc reports are in DESIGN section 7.
#include "assoc_stage.h"

#pragma clang fp contract(off)

namespace gpca {

struct AsgSmem {
    uint8_t g[2][kAsgMaxRows * kAscGPitch];
    float w[2][kAscStage];
    unsigned sums[kAsgMaxRows * 2];
};

// lrows [listed]: the original row of every listed row; sums [listed][3]: the count kernel's; Bt: the score scan's panel (row t = w_t);
// phi: R_ab of every (strip, trait) entry at asg_phi_index
template <bool PACKED>
__global__ __launch_bounds__(kAsgThreads) void k_assoc_set_gram(const void* __restrict__ Gv, int64_t ldr, const int64_t* __restrict__ lrows,
                                                                int64_t N, int64_t npad, const float* __restrict__ Bt,
                                                                const unsigned* __restrict__ incw, const unsigned* __restrict__ sums,
                                                                const AsgStrip* __restrict__ strips, double* __restrict__ phi) {
    __shared__ __attribute__((aligned(16))) AsgSmem sm;
    const uint8_t* G = (const uint8_t*)Gv;
    const AsgStrip sp = strips[blockIdx.x];
    const int t = blockIdx.y;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;

    // (the score scan's staging map: this thread stages half sh of the set's row srow)
    const int srow = threadIdx.x >> 1, sh = threadIdx.x & 1;
    const bool slive = srow < asg_staged_rows(sp.m, sp.s);
    const int64_t sorow = slive ? lrows[sp.l0 + srow] : -1;
    const unsigned snobs = slive ? sums[(sp.l0 + srow) * 3] : 0u, ss1 = slive ? sums[(sp.l0 + srow) * 3 + 1] : 0u;
    const bool flip = ss1 > snobs;
    if (sh == 0) { sm.sums[2 * srow] = snobs; sm.sums[2 * srow + 1] = flip ? 2u * snobs - ss1 : ss1; }
    const float* wt = Bt + (int64_t)asr_col_w(t) * npad;
    const bool wlive = threadIdx.x < kAscStage / 4;
    auto inb_of = [&](int64_t s) { return asc_inb(N, s * kAscStage + 32 * sh); };
    auto inc_of = [&](int64_t s) { return incw[s * (kAscStage / 32) + sh]; };

    f32x16 axx, axm, amx, amm;
    double rxx[16], rxm[16], rmx[16], rmm[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) { axx[e] = axm[e] = amx[e] = amm[e] = 0.0f; rxx[e] = rxm[e] = rmx[e] = rmm[e] = 0.0; }

    const int64_t nst = asc_stages(N);
    const bool active = wv <= sp.s;                                                  // (wave-uniform)
    const int a_off = (kAsgStripRows * sp.s + c) * kAscGPitch + 8 * h, b_off = (kAsgStripRows * wv + c) * kAscGPitch + 8 * h;
    const int sg_off = srow * kAscGPitch + 32 * sh;

    AscFetch F;
    f32x4 W = {0.0f, 0.0f, 0.0f, 0.0f};
    // (a fetch at sample ns < npad, a multiple of 32, stays inside the row's pitch; the w column holds npad floats)
    asc_fetch<PACKED>(F, G, ldr, sorow, 32 * sh);
    if (wlive) W = *reinterpret_cast<const f32x4*>(wt + 4 * threadIdx.x);
    asr_put(F, inb_of(0), inc_of(0), flip, sm.g[0] + sg_off);
    if (wlive) *reinterpret_cast<f32x4*>(sm.w[0] + 4 * threadIdx.x) = W;
    if (nst > 1) {
        asc_fetch<PACKED>(F, G, ldr, sorow, kAscStage + 32 * sh);
        if (wlive) W = *reinterpret_cast<const f32x4*>(wt + kAscStage + 4 * threadIdx.x);
    }
    __syncthreads();
    for (int64_t s = 0; s < nst; ++s) {
        if (active) {
            const uint8_t* la = sm.g[s & 1] + a_off;
            const uint8_t* lb = sm.g[s & 1] + b_off;
            const float* lw = sm.w[s & 1] + 8 * h;
#pragma unroll
            for (int q = 0; q < kAscStage / 16; ++q) {
                const uint2 ga = *reinterpret_cast<const uint2*>(la + 16 * q);
                const uint2 gb = *reinterpret_cast<const uint2*>(lb + 16 * q);
                const f32x4 w0 = *reinterpret_cast<const f32x4*>(lw + 16 * q);
                const f32x4 w1 = *reinterpret_cast<const f32x4*>(lw + 16 * q + 4);
                const bool anya = __builtin_amdgcn_ballot_w64(((ga.x | ga.y) & 0x80808080u) != 0u) != 0ull;      // wave-uniform
                const bool anyb = __builtin_amdgcn_ballot_w64(((gb.x | gb.y) & 0x80808080u) != 0u) != 0ull;
                const unsigned amx_ = (ga.x >> 7) & 0x01010101u, amy_ = (ga.y >> 7) & 0x01010101u;
                const unsigned bmx_ = (gb.x >> 7) & 0x01010101u, bmy_ = (gb.y >> 7) & 0x01010101u;
                const unsigned agx = ga.x & ~(amx_ * 0xffu), agy = ga.y & ~(amy_ * 0xffu);
                const unsigned bgx = gb.x & ~(bmx_ * 0xffu), bgy = gb.y & ~(bmy_ * 0xffu);
                float xa[8], ma[8], bx[8], bm[8];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    xa[i] = (float)((agx >> (8 * i)) & 0xffu); xa[4 + i] = (float)((agy >> (8 * i)) & 0xffu);
                    ma[i] = (float)((amx_ >> (8 * i)) & 0xffu); ma[4 + i] = (float)((amy_ >> (8 * i)) & 0xffu);
                    // (w times 0, 1 or 2: exact)
                    bx[i] = w0[i] * (float)((bgx >> (8 * i)) & 0xffu); bx[4 + i] = w1[i] * (float)((bgy >> (8 * i)) & 0xffu);
                    bm[i] = w0[i] * (float)((bmx_ >> (8 * i)) & 0xffu); bm[4 + i] = w1[i] * (float)((bmy_ >> (8 * i)) & 0xffu);
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) axx = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[i], bx[i], axx, 0, 0, 0);
                if (anyb) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) axm = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[i], bm[i], axm, 0, 0, 0);
                }
                if (anya) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) amx = __builtin_amdgcn_mfma_f32_32x32x2f32(ma[i], bx[i], amx, 0, 0, 0);
                    if (anyb) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) amm = __builtin_amdgcn_mfma_f32_32x32x2f32(ma[i], bm[i], amm, 0, 0, 0);
                    }
                }
            }
            if ((s + 1) % (kAscFlush / kAscStage) == 0 || s + 1 == nst) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    rxx[e] += (double)axx[e]; axx[e] = 0.0f;
                    rxm[e] += (double)axm[e]; axm[e] = 0.0f;
                    rmx[e] += (double)amx[e]; amx[e] = 0.0f;
                    rmm[e] += (double)amm[e]; amm[e] = 0.0f;
                }
            }
        }
        if (s + 1 < nst) {
            asr_put(F, inb_of(s + 1), inc_of(s + 1), flip, sm.g[(s + 1) & 1] + sg_off);
            if (wlive) *reinterpret_cast<f32x4*>(sm.w[(s + 1) & 1] + 4 * threadIdx.x) = W;
        }
        if (s + 2 < nst) {
            asc_fetch<PACKED>(F, G, ldr, sorow, (s + 2) * kAscStage + 32 * sh);
            if (wlive) W = *reinterpret_cast<const f32x4*>(wt + (s + 2) * kAscStage + 4 * threadIdx.x);
        }
        __syncthreads();
    }
    if (!active) return;

    // (sm.sums was written before the first barrier: n_obs and the operand's sum of every staged row)
    const int b = kAsgStripRows * wv + c;
    const double xbar_b = b < sp.m ? (double)sm.sums[2 * b + 1] / (double)sm.sums[2 * b] : 0.0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int a = acc_row(kAsgStripRows * sp.s, e, h);
        if (a >= sp.m || b > a) continue;
        const double xbar_a = (double)sm.sums[2 * a + 1] / (double)sm.sums[2 * a];
        phi[asg_phi_index(sp.p0, sp.m, t, a, b)] = (rxx[e] + (xbar_b * rxm[e] + xbar_a * rmx[e])) + (xbar_a * xbar_b) * rmm[e];
    }
}

int launch_assoc_set_gram(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* lrows, int64_t N, const float* Bt,
                          const unsigned* incw, int T, const unsigned* sums, const AsgStrip* strips, int64_t n_strips, double* phi) {
    if (n_strips <= 0) return 0;
    if (T < 1 || T > 65535 || n_strips >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)n_strips, (unsigned)T), blk(kAsgThreads);
    const int64_t npad = asc_npad(N);
    if (packed) hipLaunchKernelGGL((k_assoc_set_gram<true>), grid, blk, 0, st, G, ldr, lrows, N, npad, Bt, incw, sums, strips, phi);
    else hipLaunchKernelGGL((k_assoc_set_gram<false>), grid, blk, 0, st, G, ldr, lrows, N, npad, Bt, incw, sums, strips, phi);
    return 0;
}

// a workgroup per (strip, trait): Phi_ab of the strip's entries from R_ab (in place), the listed rows' dv and flips
__global__ __launch_bounds__(256) void k_assoc_set_finish(const double* __restrict__ dv, const unsigned* __restrict__ sums, int T, int Pc,
                                                          const AsgStrip* __restrict__ strips, double* __restrict__ phi) {
    const AsgStrip sp = strips[blockIdx.x];
    const int t = blockIdx.y, L = asr_cols(T, Pc), ca = asr_col_a(T, Pc, t, 0);
    const int a = kAsgStripRows * sp.s + (int)(threadIdx.x >> 3);
    if (a >= sp.m) return;
    const double* xa = dv + (sp.l0 + a) * L + ca;
    const bool fa = sums[3 * (sp.l0 + a) + 1] > sums[3 * (sp.l0 + a)];
    for (int b = threadIdx.x & 7; b <= a; b += 8) {
        const double* xb = dv + (sp.l0 + b) * L + ca;
        const bool fb = sums[3 * (sp.l0 + b) + 1] > sums[3 * (sp.l0 + b)];
        const int64_t at = asg_phi_index(sp.p0, sp.m, t, a, b);
        const double vw = phi[at] - xa[0] * xb[0];
        double q = 0.0;
        for (int j = 1; j <= Pc; ++j) q = q + xa[j] * xb[j];
        const double op = vw - q;
        phi[at] = fa != fb ? -op : op;
    }
}
int launch_assoc_set_finish(hipStream_t st, const double* dv, const unsigned* sums, int T, int Pc, const AsgStrip* strips, int64_t n_strips,
                            double* phi) {
    if (n_strips <= 0) return 0;
    if (T < 1 || T > 65535 || n_strips >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_assoc_set_finish, dim3((unsigned)n_strips, (unsigned)T), dim3(256), 0, st, dv, sums, T, Pc, strips, phi);
    return 0;
}

}  // namespace gpca
