// Linear association scan (gpca_assoc_linear; gpca_assoc.cpp): ordinary least squares of T traits on (1, C, g) for every kept row g,
// a missing call imputed to the row's mean over the included samples.  (The stage pipeline lives in assoc_tile.h and the staging
// helpers in assoc_stage.h, both shared with assoc_score.hip.)
//
// The host hands over B = [Y~ | Q] (N x L, L = T + Pc <= 64, f32; every column sums to 0 over the included samples and is 0 outside
// them), transposed and zero-padded to [asc_lpad(L)][asc_npad(N)], and the include mask as one bit per sample.  With o = [observed and
// included], g' = g o:
//     n_obs = sum o,  s1 = sum g',  s2 = sum g'^2          (exact integers, counted while the calls are staged)
//     d_ij = sum_n g'_in B_nj,   e_ij = sum_n [missing and included]_in B_nj
// k_assoc: asc_pipeline (assoc_tile.h: the tile, the stages through two LDS buffers, the exact products, the order of the samples and
// the flush into f64 running sums) with asc_put as the stager: the staged bytes are the calls (0, 1, 2 or the missing code), checked
// and counted on their way into LDS.  No split of the sample axis, no atomics: a row's sums depend on the row and on N alone, so a band
// gives the bits of the full call and int8 and 2-bit residency (the same bytes in LDS) give the same bits.
// Registers, lpad = 64: d and e each hold 2 x 16 f32 accumulators and 2 x 16 f64 running sums = 96 registers, 192 for both; with the
// prefetch of a stage (8 of calls + 16 of B) and the operands of a group (16 + 16) the compiler takes 256 VGPRs + 76 AGPRs of the
// 512 a wave of a 256-thread workgroup may use (no spill): one wave per SIMD.  lpad = 32 halves the sums: 158 + 32, two waves.
// Epilogue (f64, no contraction): mbar = s1 / n_obs, xb_ij = d_ij + mbar * e_ij.  k_assoc_finish (one thread per row): xx = s2 - s1 *
// mbar, sxx = xx - sum_{j >= T} xb_ij^2 (j ascending), and per trait beta = xb / sxx, rss = yy - xb * beta, se = sqrt(rss / df / sxx),
// t = beta / se; NaN when n_obs = 0, xx <= 0, sxx * max_vif < xx or rss <= 0.
// Out of scope: case / control traits (assoc_score.hip has their score test), per-variant dropping of samples with a missing call,
// per-trait sample sets, mixed models that use the GRM, streamed and row-sharded handles.
#include "assoc_tile.h"

#pragma clang fp contract(off)

namespace gpca {

// xb [row1 - row0][L] f64, sums [row1 - row0][3] u32 of kept rows [row0, row1); *bad = min original row with a value outside
// {0, 1, 2, missing}
template <bool PACKED, int NB>
__global__ __launch_bounds__(kAscThreads) void k_assoc(const void* __restrict__ Gv, int64_t ldr, const int64_t* __restrict__ krows, int64_t N,
                                                       int64_t npad, const float* __restrict__ Bt, const unsigned* __restrict__ incw, int L,
                                                       int64_t row0, int64_t row1, double* __restrict__ xb, unsigned* __restrict__ sums,
                                                       unsigned long long* __restrict__ bad) {
    __shared__ __attribute__((aligned(16))) AscSmem<NB, 3> sm;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int64_t k0 = row0 + (int64_t)blockIdx.x * kAscRows;

    // (the pipeline's staging map: this thread stages half sh of row srow)
    const int srow = threadIdx.x >> 1, sh = threadIdx.x & 1;
    const int64_t sorow = k0 + srow < row1 ? krows[k0 + srow] : -1;
    unsigned nobs = 0u, s1 = 0u, s2 = 0u, bd = 0u;
    double rd[NB][16], re[NB][16];
    asc_pipeline<PACKED, NB, false>(sm, (const uint8_t*)Gv, ldr, sorow, N, npad, Bt, incw,
                         [&](const AscFetch& F, unsigned inb, unsigned inc, uint8_t* dst) { asc_put(F, inb, inc, dst, nobs, s1, s2, bd); }, rd, re, nullptr, wv, lane);

    if (bd && sorow >= 0) atomicMin(bad, (unsigned long long)sorow);
    // the two halves of a row sit in neighbouring lanes
    nobs += __shfl_xor(nobs, 1); s1 += __shfl_xor(s1, 1); s2 += __shfl_xor(s2, 1);
    if (sh == 0) {
        sm.sums[3 * srow] = nobs; sm.sums[3 * srow + 1] = s1; sm.sums[3 * srow + 2] = s2;
        if (sorow >= 0) {
            unsigned* o = sums + (k0 + srow - row0) * 3;
            o[0] = nobs; o[1] = s1; o[2] = s2;
        }
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int r = asc_acc_row(wv, h, e);
        const int64_t kr = k0 + r;
        if (kr >= row1) continue;
        const double mbar = (double)sm.sums[3 * r + 1] / (double)sm.sums[3 * r];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int col = 32 * j + c;
            if (col < L) xb[(kr - row0) * L + col] = rd[j][e] + mbar * re[j][e];
        }
    }
}

int launch_assoc(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t N, const float* Bt,
                 const unsigned* incw, int L, int64_t row0, int64_t row1, double* xb, unsigned* sums, unsigned long long* bad) {
    if (row1 <= row0) return 0;
    const int64_t nb = asc_row_blocks(row1 - row0);
    if (L < 1 || L > kAscMaxCols || nb >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)nb), blk(kAscThreads);
    const int64_t npad = asc_npad(N);
#define GPCA_ASC(PK, NB) hipLaunchKernelGGL((k_assoc<PK, NB>), grid, blk, 0, st, G, ldr, krows, N, npad, Bt, incw, L, row0, row1, xb, sums, bad)
    if (asc_lpad(L) == 32) { if (packed) GPCA_ASC(true, 1); else GPCA_ASC(false, 1); }
    else { if (packed) GPCA_ASC(true, 2); else GPCA_ASC(false, 2); }
#undef GPCA_ASC
    return 0;
}

// one thread per row of the band: rowinfo [rows][4] = n_obs, a1_freq, xx, sxx and stats [rows][T][3] = beta, se, t (each may be NULL)
__global__ __launch_bounds__(256) void k_assoc_finish(const double* __restrict__ xb, const unsigned* __restrict__ sums,
                                                      const double* __restrict__ yy, int T, int L, double df, double max_vif, int64_t rows,
                                                      double* __restrict__ stats, double* __restrict__ info) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const double nobs = (double)sums[3 * i], s1 = (double)sums[3 * i + 1], s2 = (double)sums[3 * i + 2];
    const double mbar = s1 / nobs;
    const double xx = s2 - s1 * mbar;
    const double* x = xb + i * L;
    double q = 0.0;
    for (int j = T; j < L; ++j) q = q + x[j] * x[j];
    const double sxx = xx - q;
    if (info) { double* o = info + 4 * i; o[0] = nobs; o[1] = mbar / 2.0; o[2] = xx; o[3] = sxx; }
    if (!stats) return;
    const bool dead = sums[3 * i] == 0u || !(xx > 0.0) || sxx * max_vif < xx;
    const double nan = __builtin_nan("");
    for (int t = 0; t < T; ++t) {
        const double beta = x[t] / sxx;
        const double rss = yy[t] - x[t] * beta;
        const double se = sqrt(rss / df / sxx);
        const bool ok = !dead && rss > 0.0;
        double* o = stats + (i * T + t) * 3;
        o[0] = ok ? beta : nan; o[1] = ok ? se : nan; o[2] = ok ? beta / se : nan;
    }
}
void launch_assoc_finish(hipStream_t st, const double* xb, const unsigned* sums, const double* yy, int T, int L, double df, double max_vif,
                         int64_t rows, double* stats, double* info) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(k_assoc_finish, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, xb, sums, yy, T, L, df, max_vif, rows, stats, info);
}

}  // namespace gpca
