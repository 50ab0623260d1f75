// f2 jackknife blocks (gpca_f2_blocks; gpca_f2_blocks.cpp; include/gpca.h section a23): for every jackknife block of rows and every
// pair of groups, the sum of the unbiased f2 of the block's rows on a 2^-40 grid and the number of rows behind it, from the counts
// workspace k_group_counts leaves on the device (counts [rows][P][3] u32 = n_obs, n_het, n_hom2).
//
// k_f2_blocks: a workgroup owns kFbRun band rows, in LDS tiles of kFbTile rows.  Per tile a wave stages one row at a time: lane g forms
//     n = 2 n_obs,  p = (n_het + 2 n_hom2) / n,  h = (p (1 - p)) / (n - 1)
// of group g in f64 (two divisions per (row, group), none per pair), and the wave's ballot of n_obs >= 1 is the row's validity mask.
// Thread t then owns the pairs t, t + kFbThreads, ... (S slots, at most kFbSlots at 64 groups) and walks the tile's rows: p_i is the
// same LDS word for most of a wave (a broadcast), p_j runs over consecutive words.  Per row and pair
//     d = p_i - p_j,  v = (d d - h_i) - h_j,  q = __double2ll_rn(v 2^40)
// with no fused multiply-add (the pragma below), which is gpca_fst_hudson's `num` bit for bit; the pair's i64 sum and i32 count stay in
// registers while the block id (the same for every thread of the workgroup: a row has one) stays the same, and go out with one 64-bit
// and one 32-bit vector atomic at a block change and at the end of the workgroup's rows.  Integer atomics: the sums do not depend on
// their order.  The figures hipcc reports are in DESIGN section 7.
#include "kernels.h"

#pragma clang fp contract(off)

namespace gpca {

struct FbSmem {
    double p[kFbTile * kFbPitch];
    double h[kFbTile * kFbPitch];
    unsigned long long mask[kFbTile];
    int blk[kFbTile];
};
static_assert(sizeof(FbSmem) == (size_t)fb_lds_bytes(), "plan_math.h: fb_lds_bytes");

template <int S>
__device__ __forceinline__ void fb_flush(long long (&sum)[S], int (&num)[S], const int (&pq)[S], int64_t b, int P,
                                         long long* __restrict__ acc, int* __restrict__ cnt) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
        if (num[s] != 0) {
            const int64_t ix = fb_out_index(b, P, pq[s]);
            atomicAdd(reinterpret_cast<unsigned long long*>(acc) + ix, (unsigned long long)sum[s]);
            atomicAdd(cnt + ix, num[s]);
        }
        sum[s] = 0; num[s] = 0;
    }
}

// counts [rows][P][3]; block [rows] in -1 .. B - 1 (checked by the host); acc [B][pairs] i64 and cnt [B][pairs] i32, zeroed by the caller
template <int S>
__global__ __launch_bounds__(kFbThreads) void k_f2_blocks(const unsigned* __restrict__ counts, const int* __restrict__ block, int64_t rows,
                                                          int P, long long* __restrict__ acc, int* __restrict__ cnt) {
    __shared__ __attribute__((aligned(16))) FbSmem sm;
    const int t = threadIdx.x, lane = t & 63;
    const int pairs = fb_pairs(P);
    const int64_t r0 = (int64_t)blockIdx.x * kFbRun;
    const int64_t rend = r0 + kFbRun < rows ? r0 + kFbRun : rows;

    // this thread's pairs: slot s holds pair t + kFbThreads s, or nothing (pq = -1)
    int pq[S], pi[S], pj[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int q = t + kFbThreads * s;
        const bool live = q < pairs;
        pq[s] = live ? q : -1;
        pi[s] = live ? fb_pair_i(q) : 1;
        pj[s] = live ? fb_pair_j(q) : 0;
    }
    long long sum[S];
    int num[S];
#pragma unroll
    for (int s = 0; s < S; ++s) { sum[s] = 0; num[s] = 0; }
    int cur = -1;                                                                   // the block of the sums in registers (-1: none)

    const int sg = fb_stage_group(t);
    for (int64_t tr0 = r0; tr0 < rend; tr0 += kFbTile) {
        const int nrow = (int)(rend - tr0 < kFbTile ? rend - tr0 : kFbTile);
        __syncthreads();                                                            // (the previous tile's readers are done)
#pragma unroll
        for (int k = 0; k < fb_stage_passes(); ++k) {
            const int r = fb_stage_row(t, k);                                       // wave-uniform
            if (r >= nrow) continue;
            double p = 0.0, hh = 0.0;
            bool ok = false;
            if (sg < P) {
                const unsigned* c = counts + gc_counts_index(tr0 + r, P, sg, 0);
                const unsigned c0 = c[0], c1 = c[1], c2 = c[2];
                if (c0 >= 1u) {
                    const double n = 2.0 * (double)c0;
                    p = ((double)c1 + 2.0 * (double)c2) / n;
                    hh = (p * (1.0 - p)) / (n - 1.0);
                    ok = true;
                }
            }
            const unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
            sm.p[fb_lds_index(r, sg)] = p;
            sm.h[fb_lds_index(r, sg)] = hh;
            if (lane == 0) { sm.mask[r] = m; sm.blk[r] = block[tr0 + r]; }
        }
        __syncthreads();
        for (int r = 0; r < nrow; ++r) {
            const int b = sm.blk[r];                                                // the same in every thread
            if (b < 0) continue;
            if (b != cur) {
                if (cur >= 0) fb_flush<S>(sum, num, pq, cur, P, acc, cnt);
                cur = b;
            }
            const unsigned long long m = sm.mask[r];
#pragma unroll
            for (int s = 0; s < S; ++s) {
                if (pq[s] < 0 || !((m >> pi[s]) & (m >> pj[s]) & 1ull)) continue;
                const int ii = fb_lds_index(r, pi[s]), jj = fb_lds_index(r, pj[s]);
                const double d = sm.p[ii] - sm.p[jj];
                const double v = (d * d - sm.h[ii]) - sm.h[jj];
                sum[s] += __double2ll_rn(v * kFbScale);
                num[s] += 1;
            }
        }
    }
    if (cur >= 0) fb_flush<S>(sum, num, pq, cur, P, acc, cnt);
}

int launch_f2_blocks(hipStream_t st, const unsigned* counts, const int* block, int64_t rows, int P, long long* acc, int* cnt) {
    if (rows <= 0) return 0;
    if (P < 2 || P > kGcMaxGroups || rows > kFbMaxRows) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)fb_row_blocks(rows)), blk(kFbThreads);
#define GPCA_FB(S) hipLaunchKernelGGL((k_f2_blocks<S>), grid, blk, 0, st, counts, block, rows, P, acc, cnt)
    const int slots = fb_slots(P);
    if (slots <= 1) GPCA_FB(1);
    else if (slots <= 2) GPCA_FB(2);
    else if (slots <= 4) GPCA_FB(4);
    else GPCA_FB(8);
#undef GPCA_FB
    return 0;
}

}  // namespace gpca
