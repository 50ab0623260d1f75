// Logistic score scan (gpca_assoc_logistic_score; gpca_assoc_score.cpp): the score test of T case / control traits for every kept row
// g, the null logistic model of each trait fitted once on the host, a missing call imputed to the row's mean over the included samples.
//
// The host hands over the panel B (N x L, L = T (Pc + 3) <= 64, f32, 0 outside the included samples S), transposed and zero-padded
// to [asc_lpad(L)][asc_npad(N)] as the linear scan's is, and the include mask as one bit per sample.  Per trait t, with mu the fitted
// probabilities, X = (1, C centred over S and scaled to unit norm) and X^T W X = L L^T:
//     w_t = mu (1 - mu)   (columns 0 .. T - 1),     r_t = y - mu   (columns T .. 2 T - 1),
//     A_t,j, j = 0 .. Pc = the columns of W X L^-T   (columns 2 T + t (Pc + 1) + j; j = 0 is the intercept's).
// k_assoc_score_count (a wave per row, a lane 32 samples of every 2 048): o = [observed and in S], the exact integers n_obs = sum o,
// s1 = sum g o, s2 = sum g^2 o, and the invalid-genotype flag.  Row i is FLIPPED iff s1 > n_obs (its A1 mean is above 1): a function
// of the row and S alone.
// k_assoc_score: asc_pipeline (assoc_tile.h: the tile and pipeline that k_assoc runs too) with asr_put as the stager and the x^2
// accumulator on.  The staged byte of a sample is the operand x = g o on a plain row and (2 - g) o on a flipped one (0, 1, 2), or the
// missing code for m = [missing and in S].  Per 16-sample group
//     d_c += x B_c   (all columns),     e_c += m B_c   (only where a wave ballot finds a missing call),     q_c += x^2 B_c   (the first
//     block of 32 columns only: it holds every w_t)
// x, m and x^2 are 0, 1, 2 or 4, so every product is exact.  No split of the sample axis, no atomics on sums: a row's sums depend on
// the row, S and N alone, so a band gives the bits of the full call and int8 and 2-bit residency (the same bytes in LDS) give the same
// bits.  A 16-sample group issues 8 NB + 8 multiplies against k_assoc's 8 NB.
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
#include "assoc_tile.h"

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
        unsigned o[8];
        asc_mask_count(F, asc_inb(N, n0), incw[n0 >> 5], o, nobs, s1, s2, bd);
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

// dv [row1 - row0][L] f64 of kept rows [row0, row1); sums: what k_assoc_score_count left for the same band
template <bool PACKED, int NB>
__global__ __launch_bounds__(kAscThreads) void k_assoc_score(const void* __restrict__ Gv, int64_t ldr, const int64_t* __restrict__ krows, int64_t N,
                                                             int64_t npad, const float* __restrict__ Bt, const unsigned* __restrict__ incw, int T,
                                                             int L, int64_t row0, int64_t row1, const unsigned* __restrict__ sums,
                                                             double* __restrict__ dv) {
    __shared__ __attribute__((aligned(16))) AscSmem<NB, 2> sm;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int64_t k0 = row0 + (int64_t)blockIdx.x * kAscRows;

    // (the pipeline's staging map: this thread stages half sh of row srow)
    const int srow = threadIdx.x >> 1, sh = threadIdx.x & 1;
    const bool slive = k0 + srow < row1;
    const int64_t sorow = slive ? krows[k0 + srow] : -1;
    const unsigned snobs = slive ? sums[(k0 + srow - row0) * 3] : 0u, ss1 = slive ? sums[(k0 + srow - row0) * 3 + 1] : 0u;
    const bool flip = ss1 > snobs;
    if (sh == 0) { sm.sums[2 * srow] = snobs; sm.sums[2 * srow + 1] = flip ? 2u * snobs - ss1 : ss1; }
    double rd[NB][16], re[NB][16], rq[16];
    asc_pipeline<PACKED, NB, true>(sm, (const uint8_t*)Gv, ldr, sorow, N, npad, Bt, incw,
                         [&](const AscFetch& F, unsigned inb, unsigned inc, uint8_t* dst) { asr_put(F, inb, inc, flip, dst); }, rd, re, rq, wv, lane);

    // (sm.sums was written before the first barrier: n_obs and the operand's sum of every row of the tile)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int r = asc_acc_row(wv, h, e);
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
