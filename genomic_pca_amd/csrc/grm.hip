// Genetic relationship matrix (gpca_grm, gpca_grm.cpp): a lower-triangular symmetric rank-K update over the kept SNP rows.
//
//   K . GRM[a][b] = sum_i Z[i][a] Z[i][b],   Z = r g' + b p   (g' = the call, 0 where missing; p = 1 - m, m = the missing indicator)
//                 = sum_i w g'_a g'_b + c (g'_a m_b + m_a g'_b) + e m_a m_b  -  (u_a + u_b)  +  beta  -  (v_a + v_b)
// with w = r^2, c = -r b >= 0, e = b^2 >= 0, u_a = sum_i c g'_a, v_a = sum_i e m_a, beta = sum_i e (centred scaling: r = 1, b = -mu).
// The first sum is the matrix-core work: A = g' (or m, or digits of c o m) of the row-side samples, B = base-128 digit planes of the
// column side's w o g' (or c o m, e o m), all four tables quantised on ONE power-of-two scale S chosen by the host (gpca_grm.cpp).
// For a given row and pair (a, b) exactly one of the four products is nonzero, so they share one set of i32 accumulators per digit
// plane: |partial| <= 2 * 127 per row.  The digits of w g' come from a per-row table of the digits of w and of 2w (one v_perm per
// dword and plane, the selector built once per block from g'); blocks without a missing call (wave ballot) run the w o g' planes only.
// The vectors u, v, the counts and the dosage check come from k_grm_vec (one read of every genotype).
//
// Workgroup = one 64 x 64 tile (tile row >= tile column) of the output; four waves of 32 x 32.  Every 32-row block of both sample
// ranges is staged through LDS transposed to [sample][row], so that a lane reads its 16 k-contiguous bytes with one ds_read_b128;
// the global loads of the next block are issued before the current one is multiplied.
// Integer partials are flushed to an f64 running sum once per kGrmFlushRows rows counted from the panel's first row, in row order, and
// the running sums live in the caller's buffer between panels: the bits do not depend on the launch grid, the band or (when the panel
// rows are a multiple of kGrmFlushRows) the panels.
#include "syrk_tile.h"

namespace gpca {

static_assert(kGrmFlushRows % 32 == 0 && (int64_t)kGrmFlushRows * 254 < ((int64_t)1 << 31), "flush group");
constexpr int kGrmLdsPitch = 48;      // bytes per sample of a staged block (32 rows + 16: ds_read_b128 stays 16-byte aligned)

// Staging of block `blk` of the two sample ranges, in two halves so that the global loads of block blk + 1 are in flight while the
// waves multiply block blk: thread t < 128 loads side a, t >= 128 side b, (rq, cq) = 4 rows x 4 samples; t < 48 also loads the tables.
struct GrmFetch { unsigned x[4]; i32x4 t; };
template <bool PACKED>
__device__ __forceinline__ void grm_fetch(GrmFetch& F, const uint8_t* __restrict__ G, int64_t ldr, int64_t blk, int64_t ca0, int64_t cb0,
                                          const int8_t* __restrict__ tab) {
    const int t = threadIdx.x, side = t >> 7, u = t & 127, rq = u >> 4, cq = u & 15;
    const int64_t col = (side ? cb0 : ca0) + 4 * cq;
    unit_fetch<PACKED>(F.x, G + (blk * 32 + 4 * rq) * ldr + (PACKED ? col / 4 : col), ldr);
    if (t < kGrmTabBytes / 16) F.t = *reinterpret_cast<const i32x4*>(tab + blk * kGrmTabBytes + 16 * t);
}
template <bool PACKED>
__device__ __forceinline__ void grm_put(const GrmFetch& F, uint8_t* la, uint8_t* lb, uint8_t* lt) {
    const int t = threadIdx.x, side = t >> 7, u = t & 127, rq = u >> 4, cq = u & 15;
    unit_put<PACKED>(F.x, (side ? lb : la) + (4 * cq) * kGrmLdsPitch + 4 * rq, kGrmLdsPitch);
    if (t < kGrmTabBytes / 16) *reinterpret_cast<i32x4*>(lt + 16 * t) = F.t;
}

// R [band]: running f64 sums of the digit-combined integer partials (unscaled); Q [band]: sum over kept rows of m_a m_b.
// Band element (a, b <= a), row0 <= a < row1, a < N, at band_index(row0, a, b, true).  first: R and Q start at 0.
template <bool PACKED>
__global__ __launch_bounds__(256, 1) void k_grm(const void* __restrict__ Gv, int64_t ldr, int64_t rows_pad, const int8_t* __restrict__ tab,
                                                 const uint32_t* __restrict__ kmask, const int2* __restrict__ tiles, int64_t row0,
                                                 int64_t row1, int64_t N, double* __restrict__ R, int* __restrict__ Q, int first) {
    __shared__ __attribute__((aligned(16))) uint8_t la[kGrmTile * kGrmLdsPitch];
    __shared__ __attribute__((aligned(16))) uint8_t lb[kGrmTile * kGrmLdsPitch];
    __shared__ __attribute__((aligned(16))) uint8_t lt[kGrmTabBytes];
    const uint8_t* G = (const uint8_t*)Gv;
    const int2 tl = tiles[blockIdx.x];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5, wa = wv >> 1, wb = wv & 1;
    const int64_t ca0 = (int64_t)tl.x * kGrmTile, cb0 = (int64_t)tl.y * kGrmTile;
    const bool active = !(tl.x == tl.y && wa == 0 && wb == 1);   // (the upper sub-tile of a diagonal tile)
    constexpr int ND = kGrmDigits;

    i32x16 acc[ND], q0;
    double run[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) { q0[e] = 0; run[e] = 0.0; }
    const int64_t a_base = ca0 + 32 * wa, b_col = cb0 + 32 * wb + c;
    const int64_t base = band_entries(0, row0, true);
    if (!first && active && b_col < N) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int64_t a = acc_row(a_base, e, h);
            if (band_holds<true>(row0, row1, N, a, b_col)) { const int64_t ix = band_entries(0, a, true) - base + b_col; run[e] = R[ix]; q0[e] = Q[ix]; }
        }
    }
    const int64_t nblk = rows_pad >> 5;
    GrmFetch F;
    grm_fetch<PACKED>(F, G, ldr, 0, ca0, cb0, tab);
    for (int64_t g0 = 0; g0 < nblk; g0 += kGrmFlushRows / 32) {
        const int64_t g1 = g0 + kGrmFlushRows / 32 < nblk ? g0 + kGrmFlushRows / 32 : nblk;
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[d][e] = 0;
        for (int64_t blk = g0; blk < g1; ++blk) {
            __syncthreads();                                   // the previous block's readers are done with the LDS
            grm_put<PACKED>(F, la, lb, lt);
            __syncthreads();
            if (blk + 1 < nblk) grm_fetch<PACKED>(F, G, ldr, blk + 1, ca0, cb0, tab);   // in flight while this block is multiplied
            if (!active) continue;
            const i32x4 xa = *reinterpret_cast<const i32x4*>(la + (32 * wa + c) * kGrmLdsPitch + 16 * h);
            const i32x4 xb = *reinterpret_cast<const i32x4*>(lb + (32 * wb + c) * kGrmLdsPitch + 16 * h);
            i32x4 ga, ma, gb, mb, sel;
            unsigned anym = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned va = (unsigned)xa[k], vb = (unsigned)xb[k];
                const unsigned mA = (va >> 7) & 0x01010101u, mB = (vb >> 7) & 0x01010101u;
                const unsigned gA = va & ~(mA * 0xffu), gB = vb & ~(mB * 0xffu);
                ma[k] = (int)mA; mb[k] = (int)mB; ga[k] = (int)gA; gb[k] = (int)gB;
                anym |= mA | mB;
                // v_perm selector of the w o g' digits: g' = 1 -> byte k of the w plane, 2 -> byte k of the 2w plane, 0 -> 0x00
                const unsigned two = (gB >> 1) & 0x01010101u, z = ((gB | (gB >> 1)) & 0x01010101u) ^ 0x01010101u;
                sel[k] = (int)(((0x03020100u + two * 4u) & ~(z * 0xffu)) | (z * 0x0cu));
            }
            const bool miss = __builtin_amdgcn_ballot_w64(anym != 0u) != 0ull;   // wave-uniform
            const int8_t* tw1 = (const int8_t*)lt + 16 * h;
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                const i32x4 t1 = *reinterpret_cast<const i32x4*>(tw1 + (0 * ND + d) * 32);
                const i32x4 t2 = *reinterpret_cast<const i32x4*>(tw1 + (1 * ND + d) * 32);
                i32x4 bw;
#pragma unroll
                for (int k = 0; k < 4; ++k) bw[k] = permb(t2[k], t1[k], (unsigned)sel[k]);
                if (miss) {
                    const i32x4 tc = *reinterpret_cast<const i32x4*>(tw1 + (2 * ND + d) * 32);
#pragma unroll
                    for (int k = 0; k < 4; ++k) bw[k] |= tc[k] & (int)((unsigned)mb[k] * 0xffu);
                }
                acc[d] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ga, bw, acc[d], 0, 0, 0);
            }
            if (miss) {
#pragma unroll
                for (int d = 0; d < ND; ++d) {
                    const i32x4 tc = *reinterpret_cast<const i32x4*>(tw1 + (2 * ND + d) * 32);
                    const i32x4 te = *reinterpret_cast<const i32x4*>(tw1 + (3 * ND + d) * 32);
                    i32x4 ac, be;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        ac[k] = tc[k] & (int)((unsigned)ma[k] * 0xffu);
                        be[k] = te[k] & (int)((unsigned)mb[k] * 0xffu);
                    }
                    acc[d] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ac, gb, acc[d], 0, 0, 0);
                    acc[d] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ma, be, acc[d], 0, 0, 0);
                }
                // NPAIRS: the indicator of the row side restricted to kept rows (the tables are 0 on the other rows already)
                const unsigned km = (kmask[blk] >> (16 * h)) & 0xffffu;
                i32x4 mk;
#pragma unroll
                for (int k = 0; k < 4; ++k) mk[k] = (int)((unsigned)ma[k] & kept_bytes(km, k));
                q0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(mk, mb, q0, 0, 0, 0);
            }
        }
        if (active) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                double s = (double)acc[ND - 1][e];
#pragma unroll
                for (int d = ND - 2; d >= 0; --d) s = fma(s, 128.0, (double)acc[d][e]);
                run[e] += s;
            }
        }
    }
    if (!active || b_col >= N) return;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int64_t a = acc_row(a_base, e, h);
        if (band_holds<true>(row0, row1, N, a, b_col)) { const int64_t ix = band_entries(0, a, true) - base + b_col; R[ix] = run[e]; Q[ix] = q0[e]; }
    }
}

void launch_grm(hipStream_t st, const void* G, int packed, int64_t ldr, int64_t rows_pad, const int8_t* tab, const uint32_t* kmask,
                const int2* tiles, int64_t ntiles, int64_t row0, int64_t row1, int64_t N, double* R, int* Q, int first) {
    if (ntiles <= 0) return;
    if (packed) hipLaunchKernelGGL(k_grm<true>, dim3((unsigned)ntiles), dim3(256), 0, st, G, ldr, rows_pad, tab, kmask, tiles, row0, row1, N, R, Q, first);
    else hipLaunchKernelGGL(k_grm<false>, dim3((unsigned)ntiles), dim3(256), 0, st, G, ldr, rows_pad, tab, kmask, tiles, row0, row1, N, R, Q, first);
}

// Per sample n and flush group of the panel: U = sum qc_i g'_in, V = sum qe_i m_in over kept rows (exact in int64), cnt += kept rows
// missing in n, bad |= 1 for a kept row holding a value outside {0, 1, 2, -127}.  Up / Vp [ngroups][Npad].
template <bool PACKED>
__global__ __launch_bounds__(256) void k_grm_vec(const void* __restrict__ Gv, int64_t ldr, int64_t rows, int64_t Npad,
                                                 const uint8_t* __restrict__ keep, const int64_t* __restrict__ qc, const int64_t* __restrict__ qe,
                                                 double* __restrict__ Up, double* __restrict__ Vp, unsigned* __restrict__ cnt, unsigned* __restrict__ bad) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t gi = blockIdx.y;
    if (n >= Npad) return;
    const uint8_t* G = (const uint8_t*)Gv;
    const int64_t i0 = gi * kGrmFlushRows, i1 = i0 + kGrmFlushRows < rows ? i0 + kGrmFlushRows : rows;
    long long su = 0, sv = 0;
    unsigned nm = 0, bd = 0;
    for (int64_t i = i0; i < i1; ++i) {
        if (!keep[i]) continue;
        const unsigned v = call_at<PACKED>(G, ldr, i, n);
        if (v == kMissingByte) { ++nm; sv += qe[i]; }
        else if (v <= 2u) su += (long long)v * qc[i];
        else bd = 1u;
    }
    Up[gi * Npad + n] = (double)su;
    Vp[gi * Npad + n] = (double)sv;
    if (nm) atomicAdd(cnt + n, nm);
    if (bd) atomicOr(bad, 1u);
}
void launch_grm_vec(hipStream_t st, const void* G, int packed, int64_t ldr, int64_t rows, int64_t Npad, const uint8_t* keep,
                    const int64_t* qc, const int64_t* qe, double* Up, double* Vp, unsigned* cnt, unsigned* bad) {
    const int64_t ng = (rows + kGrmFlushRows - 1) / kGrmFlushRows;
    if (ng <= 0) return;
    const dim3 grid((unsigned)((Npad + 255) / 256), (unsigned)ng);
    if (packed) hipLaunchKernelGGL(k_grm_vec<true>, grid, dim3(256), 0, st, G, ldr, rows, Npad, keep, qc, qe, Up, Vp, cnt, bad);
    else hipLaunchKernelGGL(k_grm_vec<false>, grid, dim3(256), 0, st, G, ldr, rows, Npad, keep, qc, qe, Up, Vp, cnt, bad);
}
// u[n] += Up[g][n], v[n] += Vp[g][n] for g = 0, 1, ... in order (the running sums of every sample over the call's groups)
__global__ __launch_bounds__(256) void k_grm_vec_fold(const double* __restrict__ Up, const double* __restrict__ Vp, int64_t ng, int64_t Npad,
                                                      double* __restrict__ u, double* __restrict__ v) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= Npad) return;
    double su = u[n], sv = v[n];
    for (int64_t g = 0; g < ng; ++g) { su += Up[g * Npad + n]; sv += Vp[g * Npad + n]; }
    u[n] = su; v[n] = sv;
}
void launch_grm_vec_fold(hipStream_t st, const double* Up, const double* Vp, int64_t rows, int64_t Npad, double* u, double* v) {
    const int64_t ng = (rows + kGrmFlushRows - 1) / kGrmFlushRows;
    hipLaunchKernelGGL(k_grm_vec_fold, dim3((unsigned)((Npad + 255) / 256)), dim3(256), 0, st, Up, Vp, ng, Npad, u, v);
}

// out[ix] = S (R - u_a - u_b + beta - v_a - v_b) for the band's rows (one workgroup per row); npairs (may be NULL) = K - cnt_a - cnt_b + Q
__global__ __launch_bounds__(256) void k_grm_finish(const double* __restrict__ R, const int* __restrict__ Q, const double* __restrict__ u,
                                                    const double* __restrict__ v, const unsigned* __restrict__ cnt, double S, double beta,
                                                    double K, int64_t row0, double* __restrict__ out, double* __restrict__ npairs) {
    const int64_t a = row0 + blockIdx.x;
    const int64_t o = band_index(row0, a, 0, true);
    for (int64_t b = threadIdx.x; b <= a; b += 256) {
        out[o + b] = S * ((((R[o + b] - u[a]) - u[b]) + beta) - v[a] - v[b]);
        if (npairs) npairs[o + b] = (K - (double)cnt[a] - (double)cnt[b]) + (double)Q[o + b];
    }
}
void launch_grm_finish(hipStream_t st, const double* R, const int* Q, const double* u, const double* v, const unsigned* cnt, double S,
                       double beta, double K, int64_t row0, int64_t row1, double* out, double* npairs) {
    if (row1 <= row0) return;
    hipLaunchKernelGGL(k_grm_finish, dim3((unsigned)(row1 - row0)), dim3(256), 0, st, R, Q, u, v, cnt, S, beta, K, row0, out, npairs);
}

}  // namespace gpca
