// Logistic score scan (gpca_assoc_logistic_score; gpca_assoc_score.cpp): the score test of T case / control traits for every kept row
// g, the null logistic model of each trait fitted once on the host, a missing call imputed to the row's mean over the included samples.
//
// The host hands over the panel B (N x L, L = T (Pc + 3) <= 64, f32, 0 outside the included samples S), transposed and zero-padded
// to [asc_lpad(L)][asc_npad(N)] as k_assoc's is, and the include mask as one bit per sample.  Per trait t, with mu the fitted
// probabilities, X = (1, C centred over S and scaled to unit norm) and X^T W X = L L^T:
//     w_t = mu (1 - mu)   (columns 0 .. T - 1),     r_t = y - mu   (columns T .. 2 T - 1),
//     A_t,j, j = 0 .. Pc = the columns of W X L^-T   (columns 2 T + t (Pc + 1) + j; j = 0 is the intercept's).
// k_assoc_score_count (a wave per row, a lane 32 samples of every 2 048): o = [observed and in S], the exact integers n_obs = sum o,
// s1 = sum g o, s2 = sum g^2 o, and the invalid-genotype flag.  Row i is FLIPPED iff s1 > n_obs (its A1 mean is above 1): a function
// of the row and S alone.
// k_assoc_score: k_assoc's tile and pipeline (a workgroup owns kAscRows = 128 kept rows x all columns, 4 waves of 32 rows, stages of
// kAscStage = 64 samples through two LDS buffers, one barrier per stage; see assoc.hip).  The staged byte of a sample is the operand
// x = g o on a plain row and (2 - g) o on a flipped one (0, 1, 2), or the missing code for m = [missing and in S].  Per 16-sample group
//     d_c += x B_c   (all columns),     e_c += m B_c   (only where a wave ballot finds a missing call),     q_c += x^2 B_c   (the first
//     block of 32 columns only: it holds every w_t)
// on v_mfma_f32_32x32x2_f32; x, m and x^2 are 0, 1, 2 or 4, so every product is exact.  Every kAscFlush = 256 samples, counted from
// sample 0, the f32 accumulators are added to f64 running sums held in registers.  No split of the sample axis, no atomics on sums: a
// row's sums depend on the row, S and N alone, so a band gives the bits of the full call and int8 and 2-bit residency (the same bytes
// in LDS) give the same bits.  A 16-sample group issues 8 NB + 8 multiplies against k_assoc's 8 NB.
// Registers: d and e as in k_assoc (lpad = 64: 2 x (32 f32 + 32 f64) each), q adds 16 f32 + 16 f64; the figures hipcc reports are in
// DESIGN section 7 (no spill at either width).
// Epilogue (f64, no contraction): xbar = (s1 or 2 n_obs - s1) / n_obs, the operand's mean; dv_c = d_c + xbar e_c for c >= T (U_t and
// a_t,j), and dv_t = q_t + (xbar xbar) e_t for c = t < T (gwg_t).  k_assoc_score_finish (one thread per row): vw = gwg - a_0^2,
// V = vw - sum_{j = 1 .. Pc} a_j^2 (j ascending), s = -1 on a flipped row, beta = s U / V, se = 1 / sqrt(V), z = s U / sqrt(V),
// a1_freq = (s1 / n_obs) / 2, xx = s2 - s1 (s1 / n_obs); beta, se, z are NaN when n_obs = 0, xx <= 0, !(V > 0) or V max_vif < vw.
// Why the flip: V does not change under g -> 2 - g (the projection annihilates constants), but gwg - a_0^2 cancels by about
// (2pq + 4p^2) / (2pq), 200 at an A1 frequency of 0.99, against f32 sums of relative error (F + 3) u; with the operand's mean at most
// 1 the factor stays near 3.
// Out of scope: Firth's correction (assoc_spa.hip has the saddle-point correction), a Wald / IRLS fit per SNP, per-variant dropping of samples, case / control
// frequency columns, mixed models, streamed and row-sharded handles.
#include "assoc_stage.h"

#pragma clang fp contract(off)

namespace gpca {

// sums [row1 - row0][3] u32 = n_obs, s1, s2 of kept rows [row0, row1); *bad = min original row with a value outside {0, 1, 2, missing}
template <bool PACKED>
__global__ __launch_bounds__(kAsrCountThreads) void k_assoc_score_count(const void* __restrict__ Gv, int64_t ldr, const int64_t* __restrict__ krows,
                                                                        int64_t N, const unsigned* __restrict__ incw, int64_t row0, int64_t row1,
                                                                        unsigned* __restrict__ sums, unsigned long long* __restrict__ bad) {
    const uint8_t* G = (const uint8_t*)Gv;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t kr = row0 + (int64_t)blockIdx.x * kAsrCountRows + wv;
    if (kr >= row1) return;                                   // (wave-uniform)
    const int64_t orow = krows[kr], npad = asc_npad(N);
    unsigned nobs = 0u, s1 = 0u, s2 = 0u, bd = 0u;
    // (n0 is a multiple of 32 below npad: the read stays inside the row's pitch and the include word exists, as in k_assoc)
    for (int64_t n0 = 32 * lane; n0 < npad; n0 += kAsrChunk) {
        AscFetch F;
        asc_fetch<PACKED>(F, G, ldr, orow, n0);
        const int64_t left = N - n0;
        const unsigned inb = left >= 32 ? 0xffffffffu : (left <= 0 ? 0u : (1u << (int)left) - 1u);
        unsigned o[8];
        asc_mask_count(F, inb, incw[n0 >> 5], o, nobs, s1, s2, bd);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        nobs += __shfl_xor(nobs, d); s1 += __shfl_xor(s1, d); s2 += __shfl_xor(s2, d); bd |= __shfl_xor(bd, d);
    }
    if (lane == 0) {
        unsigned* o = sums + (kr - row0) * 3;
        o[0] = nobs; o[1] = s1; o[2] = s2;
        if (bd) atomicMin(bad, (unsigned long long)orow);
    }
}

template <int NB>
struct AsrSmem {
    uint8_t g[2][kAscRows * kAscGPitch];
    float b[2][NB * 32 * kAscBPitch];
    unsigned sums[kAscRows * 2];
};

// dv [row1 - row0][L] f64 of kept rows [row0, row1); sums: what k_assoc_score_count left for the same band
template <bool PACKED, int NB>
__global__ __launch_bounds__(kAscThreads) void k_assoc_score(const void* __restrict__ Gv, int64_t ldr, const int64_t* __restrict__ krows, int64_t N,
                                                             int64_t npad, const float* __restrict__ Bt, const unsigned* __restrict__ incw, int T,
                                                             int L, int64_t row0, int64_t row1, const unsigned* __restrict__ sums,
                                                             double* __restrict__ dv) {
    __shared__ __attribute__((aligned(16))) AsrSmem<NB> sm;
    const uint8_t* G = (const uint8_t*)Gv;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int64_t k0 = row0 + (int64_t)blockIdx.x * kAscRows;

    // staging map: thread t carries 32 samples (half sh of the stage) of row t / 2
    const int srow = threadIdx.x >> 1, sh = threadIdx.x & 1;
    const bool slive = k0 + srow < row1;
    const int64_t sorow = slive ? krows[k0 + srow] : -1;
    const unsigned snobs = slive ? sums[(k0 + srow - row0) * 3] : 0u, ss1 = slive ? sums[(k0 + srow - row0) * 3 + 1] : 0u;
    const bool flip = ss1 > snobs;
    if (sh == 0) { sm.sums[2 * srow] = snobs; sm.sums[2 * srow + 1] = flip ? 2u * snobs - ss1 : ss1; }
    auto inb_of = [&](int64_t s) {
        const int64_t left = N - (s * kAscStage + 32 * sh);
        return left >= 32 ? 0xffffffffu : (left <= 0 ? 0u : (1u << (int)left) - 1u);
    };
    auto inc_of = [&](int64_t s) { return incw[s * (kAscStage / 32) + sh]; };

    f32x16 ad[NB], ae[NB], aq;
    double rd[NB][16], re[NB][16], rq[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) { aq[e] = 0.0f; rq[e] = 0.0; }
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) { ad[j][e] = 0.0f; ae[j][e] = 0.0f; rd[j][e] = 0.0; re[j][e] = 0.0; }

    const int64_t nst = asc_stages(N);
    const int g_off = (32 * wv + c) * kAscGPitch + 8 * h, b_off = c * kAscBPitch + 8 * h;
    const int sg_off = srow * kAscGPitch + 32 * sh;

    AscFetch F;
    f32x4 P[2 * NB];
    asc_fetch<PACKED>(F, G, ldr, sorow, 32 * sh);
    asc_fetch_b<NB>(P, Bt, npad, 0);
    asr_put(F, inb_of(0), inc_of(0), flip, sm.g[0] + sg_off);
    asc_put_b<NB>(P, sm.b[0]);
    if (nst > 1) { asc_fetch<PACKED>(F, G, ldr, sorow, kAscStage + 32 * sh); asc_fetch_b<NB>(P, Bt, npad, kAscStage); }
    __syncthreads();
    for (int64_t s = 0; s < nst; ++s) {
        const uint8_t* lg = sm.g[s & 1] + g_off;
        const float* lb = sm.b[s & 1] + b_off;
#pragma unroll
        for (int q = 0; q < kAscStage / 16; ++q) {
            const uint2 gb = *reinterpret_cast<const uint2*>(lg + 16 * q);
            const bool anym = __builtin_amdgcn_ballot_w64(((gb.x | gb.y) & 0x80808080u) != 0u) != 0ull;      // wave-uniform
            const unsigned mx = (gb.x >> 7) & 0x01010101u, my = (gb.y >> 7) & 0x01010101u;
            const unsigned gx = gb.x & ~(mx * 0xffu), gy = gb.y & ~(my * 0xffu);
            float gf[8], mf[8], g2[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                gf[i] = (float)((gx >> (8 * i)) & 0xffu); gf[4 + i] = (float)((gy >> (8 * i)) & 0xffu);
                mf[i] = (float)((mx >> (8 * i)) & 0xffu); mf[4 + i] = (float)((my >> (8 * i)) & 0xffu);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) g2[i] = gf[i] * gf[i];
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const f32x4 b0 = *reinterpret_cast<const f32x4*>(lb + 32 * j * kAscBPitch + 16 * q);
                const f32x4 b1 = *reinterpret_cast<const f32x4*>(lb + 32 * j * kAscBPitch + 16 * q + 4);
#pragma unroll
                for (int i = 0; i < 8; ++i) ad[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(gf[i], i < 4 ? b0[i] : b1[i - 4], ad[j], 0, 0, 0);
                if (j == 0) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) aq = __builtin_amdgcn_mfma_f32_32x32x2f32(g2[i], i < 4 ? b0[i] : b1[i - 4], aq, 0, 0, 0);
                }
                if (anym) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) ae[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(mf[i], i < 4 ? b0[i] : b1[i - 4], ae[j], 0, 0, 0);
                }
            }
        }
        if ((s + 1) % (kAscFlush / kAscStage) == 0 || s + 1 == nst) {
#pragma unroll
            for (int e = 0; e < 16; ++e) { rq[e] += (double)aq[e]; aq[e] = 0.0f; }
#pragma unroll
            for (int j = 0; j < NB; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    rd[j][e] += (double)ad[j][e]; ad[j][e] = 0.0f;
                    re[j][e] += (double)ae[j][e]; ae[j][e] = 0.0f;
                }
        }
        if (s + 1 < nst) {
            asr_put(F, inb_of(s + 1), inc_of(s + 1), flip, sm.g[(s + 1) & 1] + sg_off);
            asc_put_b<NB>(P, sm.b[(s + 1) & 1]);
        }
        if (s + 2 < nst) {
            asc_fetch<PACKED>(F, G, ldr, sorow, (s + 2) * kAscStage + 32 * sh);
            asc_fetch_b<NB>(P, Bt, npad, (s + 2) * kAscStage);
        }
        __syncthreads();
    }

    // (sm.sums was written before the first barrier: n_obs and the operand's sum of every row of the tile)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int r = 32 * wv + (e & 3) + 8 * (e >> 2) + 4 * h;
        const int64_t kr = k0 + r;
        if (kr >= row1) continue;
        const double xbar = (double)sm.sums[2 * r + 1] / (double)sm.sums[2 * r];
        const double xbar2 = xbar * xbar;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int col = 32 * j + c;
            if (col >= L) continue;
            dv[(kr - row0) * L + col] = (j == 0 && col < T) ? rq[e] + xbar2 * re[0][e] : rd[j][e] + xbar * re[j][e];
        }
    }
}

int launch_assoc_score_count(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t N, const unsigned* incw,
                             int64_t row0, int64_t row1, unsigned* sums, unsigned long long* bad) {
    if (row1 <= row0) return 0;
    const int64_t nb = asr_count_blocks(row1 - row0);
    if (nb >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)nb), blk(kAsrCountThreads);
    if (packed) hipLaunchKernelGGL((k_assoc_score_count<true>), grid, blk, 0, st, G, ldr, krows, N, incw, row0, row1, sums, bad);
    else hipLaunchKernelGGL((k_assoc_score_count<false>), grid, blk, 0, st, G, ldr, krows, N, incw, row0, row1, sums, bad);
    return 0;
}

int launch_assoc_score(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t N, const float* Bt,
                       const unsigned* incw, int T, int L, int64_t row0, int64_t row1, const unsigned* sums, double* dv) {
    if (row1 <= row0) return 0;
    const int64_t nb = asc_row_blocks(row1 - row0);
    if (T < 1 || L < 3 * T || L > kAsrMaxCols || nb >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)nb), blk(kAscThreads);
    const int64_t npad = asc_npad(N);
#define GPCA_ASR(PK, NB) hipLaunchKernelGGL((k_assoc_score<PK, NB>), grid, blk, 0, st, G, ldr, krows, N, npad, Bt, incw, T, L, row0, row1, sums, dv)
    if (asc_lpad(L) == 32) { if (packed) GPCA_ASR(true, 1); else GPCA_ASR(false, 1); }
    else { if (packed) GPCA_ASR(true, 2); else GPCA_ASR(false, 2); }
#undef GPCA_ASR
    return 0;
}

// one thread per row of the band: stats [rows][T][5] = beta, se, z, vw, V; ua [rows][T][Pc + 3] = U, gwg, a_0 .. a_Pc; info [rows][5] =
// n_obs, a1_freq, xx, flipped, 0 (each may be NULL)
__global__ __launch_bounds__(256) void k_assoc_score_finish(const double* __restrict__ dv, const unsigned* __restrict__ sums, int T, int Pc,
                                                            double max_vif, int64_t rows, double* __restrict__ stats, double* __restrict__ ua,
                                                            double* __restrict__ info) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const int L = asr_cols(T, Pc);
    const double nobs = (double)sums[3 * i], s1 = (double)sums[3 * i + 1], s2 = (double)sums[3 * i + 2];
    const bool flip = sums[3 * i + 1] > sums[3 * i];
    const double mbar = s1 / nobs;
    const double xx = s2 - s1 * mbar;
    if (info) { double* o = info + 5 * i; o[0] = nobs; o[1] = mbar / 2.0; o[2] = xx; o[3] = flip ? 1.0 : 0.0; o[4] = 0.0; }
    const double* x = dv + i * L;
    const double nan = __builtin_nan(""), sg = flip ? -1.0 : 1.0;
    for (int t = 0; t < T; ++t) {
        const double U = x[asr_col_r(T, t)], gwg = x[asr_col_w(t)];
        const double* a = x + asr_col_a(T, Pc, t, 0);
        if (ua) {
            double* o = ua + (i * T + t) * (Pc + 3);
            o[0] = U; o[1] = gwg;
            for (int j = 0; j <= Pc; ++j) o[2 + j] = a[j];
        }
        if (!stats) continue;
        const double vw = gwg - a[0] * a[0];
        double q = 0.0;
        for (int j = 1; j <= Pc; ++j) q = q + a[j] * a[j];
        const double V = vw - q;
        const bool ok = sums[3 * i] != 0u && xx > 0.0 && V > 0.0 && !(V * max_vif < vw);
        const double rt = sqrt(V);
        double* o = stats + (i * T + t) * 5;
        o[0] = ok ? sg * U / V : nan; o[1] = ok ? 1.0 / rt : nan; o[2] = ok ? sg * U / rt : nan; o[3] = vw; o[4] = V;
    }
}
void launch_assoc_score_finish(hipStream_t st, const double* dv, const unsigned* sums, int T, int Pc, double max_vif, int64_t rows,
                               double* stats, double* ua, double* info) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(k_assoc_score_finish, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, dv, sums, T, Pc, max_vif, rows, stats, ua, info);
}

}  // namespace gpca
