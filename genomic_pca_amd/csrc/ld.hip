// Windowed LD (gpca_ld_window, gpca_ld.cpp): a banded symmetric rank-N update of the kept SNP rows with themselves over the samples.
//
// Per kept row and sample, from the call g: m = [missing], g' = g on an observed call (0 on a missing one), q = g'^2.  A pair i < j
// inside the window needs sum g'_i g'_j and, where a call is missing, sum g'_i m_j, m_i g'_j, q_i m_j, m_i q_j, m_i m_j; with the
// per-row sums of g', q and m (k_ld_vec) they give n, sum x, sum y, sum xx, sum yy, sum xy of include/gpca.h (section a10) and r^2
// (k_ld_finish).  Every sum is an exact integer, so the bits depend on nothing but the counts.  gpca_ld_score (gpca_ld_score.cpp) runs the
// same sweep and reduces the planes to one integer sum per row instead (k_ld_score, at the end of this file).
//
// The sample axis is the K axis of v_mfma_i32_32x32x32_i8 and it is contiguous in both residencies, so rows go to LDS as they are
// ([row][sample], no transpose) and a lane reads its 16 k-contiguous bytes with one ds_read_b128.  Workgroup = kLdRows kept rows
// (first: i0) x one chunk of kLdCols columns of the span [i0, i0 + kLdRows + weff); wave w owns column tile w of the chunk against
// both row tiles (the column operand is decoded once for the two), and skips the pairs of tiles that do not meet the band.  In the
// chunk that starts at i0 the row side is the first half of the column side and is staged once.  Two LDS buffers: the waves
// multiply stage s from one while stage s + 1 (loaded into registers during stage s - 1) is written to the other and the global loads
// of stage s + 2 are issued: two stages in flight, one barrier per stage.  Kept rows are reached through the handle's list of
// original row indices.  When rows x chunks do not fill the device the sample axis is split over workgroups and the i32 partial sums
// meet in atomics (integer addition: any order gives the same bits).
#include "syrk_tile.h"

namespace gpca {

constexpr int kLdPitch = kLdStage + 16;                  // bytes per staged row (ds_read_b128 stays 16-byte aligned, rows spread over the banks)
constexpr int kLdStageRows = kLdRows + kLdCols;          // staged rows: the row side, then the column side
constexpr int kLdSegs = kLdStage / 16;                   // 16-sample segments per staged row
constexpr int kLdUnits = kLdStageRows * kLdSegs / kLdThreads;       // (row, segment) units per thread and stage
constexpr int kLdUnitsA = kLdRows * kLdSegs / kLdThreads;           // the first of them belong to the row side
static_assert(kLdStageRows * kLdSegs % kLdThreads == 0 && kLdRows * kLdSegs % kLdThreads == 0, "staging map");
static_assert(kLdCols / 32 == kLdThreads / 64 && kLdRows == 64, "one column tile per wave, two row tiles");

// byte mask of dword w of a 16-sample segment of which the first nvalid samples exist
__device__ __forceinline__ unsigned ld_tail_mask(int w, int nvalid) {
    const int nb = nvalid - 4 * w;
    return nb >= 4 ? 0xffffffffu : (nb <= 0 ? 0u : (1u << (8 * nb)) - 1u);
}
// the three operands of four calls: g' (0 on missing), m, q = g'^2 (bit 0 of g' stays, bit 1 moves to bit 2)
__device__ __forceinline__ void ld_ops(unsigned a, unsigned& g, unsigned& m, unsigned& q) {
    m = (a >> 7) & 0x01010101u;
    g = a & ~(m * 0xffu);
    q = (g & 0x01010101u) | ((g & 0x02020202u) << 1);
}

struct LdFetch { uint4 x[kLdUnits]; };
// src[j]: the first byte of unit j's row in the resident matrix (nullptr: past the last kept row)
template <bool PACKED>
__device__ __forceinline__ void ld_fetch(LdFetch& F, const uint8_t* const (&src)[kLdUnits], int64_t stage, int seg, int j0) {
#pragma unroll
    for (int j = 0; j < kLdUnits; ++j) {
        if (j < j0) continue;
        F.x[j] = make_uint4(0u, 0u, 0u, 0u);
        if (!src[j]) continue;
        const int64_t col = stage * kLdStage + 16 * seg;
        if (PACKED) F.x[j].x = *reinterpret_cast<const unsigned*>(src[j] + col / 4);
        else F.x[j] = *reinterpret_cast<const uint4*>(src[j] + col);
    }
}
template <bool PACKED>
__device__ __forceinline__ void ld_put(const LdFetch& F, uint8_t* buf, int64_t stage, int64_t N, int seg, int lrow0, int j0) {
    const int64_t left = N - (stage * kLdStage + 16 * seg);
    const int nvalid = left >= 16 ? 16 : (left <= 0 ? 0 : (int)left);
#pragma unroll
    for (int j = 0; j < kLdUnits; ++j) {
        if (j < j0) continue;
        uint4 v;
        if (PACKED) {
            const unsigned p = F.x[j].x;
            v = make_uint4(unpack4(p & 0xffu), unpack4((p >> 8) & 0xffu), unpack4((p >> 16) & 0xffu), unpack4(p >> 24));
        } else v = F.x[j];
        if (nvalid < 16) { v.x &= ld_tail_mask(0, nvalid); v.y &= ld_tail_mask(1, nvalid); v.z &= ld_tail_mask(2, nvalid); v.w &= ld_tail_mask(3, nvalid); }
        *reinterpret_cast<uint4*>(buf + (lrow0 + j * (kLdThreads / kLdSegs)) * kLdPitch + 16 * seg) = v;
    }
}

// W [kLdProducts][rows * wmax] (i32, zeroed by the caller): slot (t, d) = pair (row0 + t, row0 + t + 1 + d) at t * wmax + d.
// grid.x = row block + nrb * chunk, grid.y = sample split of `per` stages.
template <bool PACKED>
__global__ __launch_bounds__(kLdThreads) void k_ld(const void* __restrict__ Gv, int64_t ldr, const int64_t* __restrict__ krows, int64_t K,
                                                   int64_t N, int64_t row0, int64_t row1, const int64_t* __restrict__ win_end, int wmax,
                                                   int weff, int64_t nrb, int64_t nst, int64_t per, int atomic, int* __restrict__ W) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[2][kLdStageRows * kLdPitch];
    const uint8_t* G = (const uint8_t*)Gv;
    const int64_t rb = (int64_t)blockIdx.x % nrb, chunk = (int64_t)blockIdx.x / nrb;
    const int64_t i0 = row0 + rb * kLdRows, c0 = i0 + chunk * kLdCols;
    const int64_t s0 = (int64_t)blockIdx.y * per, s1 = s0 + per < nst ? s0 + per : nst;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const bool alias = chunk == 0;                        // the row side is the head of the column side
    const int j0 = alias ? kLdUnitsA : 0;

    // staging map: unit j of thread t = staged row t / kLdSegs + j * (kLdThreads / kLdSegs), segment t % kLdSegs
    const int seg = threadIdx.x % kLdSegs, lrow0 = threadIdx.x / kLdSegs;
    const uint8_t* src[kLdUnits];
#pragma unroll
    for (int j = 0; j < kLdUnits; ++j) {
        const int lrow = lrow0 + j * (kLdThreads / kLdSegs);
        const int64_t kr = lrow < kLdRows ? i0 + lrow : c0 + (lrow - kLdRows);
        src[j] = kr < K ? G + krows[kr] * ldr : nullptr;
    }

    // the wave's column tile against the two row tiles: tile distance T - rt must reach the band (0 <= 32 (T - rt) < weff + 32)
    const int64_t T = chunk * (kLdCols / 32) + wv;
    bool act[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) act[rt] = T >= rt && 32 * (T - rt) < (int64_t)weff + 32 && i0 + 32 * rt < row1 && c0 + 32 * wv < K;
    const bool any_act = act[0] || act[1];

    i32x16 xy[2], gm[2], mg[2], qm[2], mq[2], mm[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int e = 0; e < 16; ++e) { xy[rt][e] = 0; gm[rt][e] = 0; mg[rt][e] = 0; qm[rt][e] = 0; mq[rt][e] = 0; mm[rt][e] = 0; }
    bool saw_missing = false;
    const int a_off = ((alias ? kLdRows : 0) + c) * kLdPitch + 16 * h, b_off = (kLdRows + 32 * wv + c) * kLdPitch + 16 * h;

    LdFetch F;
    if (s0 < s1) {
        ld_fetch<PACKED>(F, src, s0, seg, j0);
        ld_put<PACKED>(F, lds[0], s0, N, seg, lrow0, j0);
        if (s0 + 1 < s1) ld_fetch<PACKED>(F, src, s0 + 1, seg, j0);
    }
    __syncthreads();
    for (int64_t s = s0; s < s1; ++s) {
        const uint8_t* buf = lds[(s - s0) & 1];
        if (any_act) {
#pragma unroll
            for (int kk = 0; kk < kLdStage / 32; ++kk) {
                const i32x4 vb = *reinterpret_cast<const i32x4*>(buf + b_off + 32 * kk);
                i32x4 GB, MB, QB, GA[2], MA[2], QA[2];
                unsigned anym = 0u;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    unsigned g, m, q;
                    ld_ops((unsigned)vb[k], g, m, q);
                    GB[k] = (int)g; MB[k] = (int)m; QB[k] = (int)q;
                    anym |= m;
                }
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) {
                    if (!act[rt]) continue;
                    const i32x4 va = *reinterpret_cast<const i32x4*>(buf + a_off + 32 * rt * kLdPitch + 32 * kk);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        unsigned g, m, q;
                        ld_ops((unsigned)va[k], g, m, q);
                        GA[rt][k] = (int)g; MA[rt][k] = (int)m; QA[rt][k] = (int)q;
                        anym |= m;
                    }
                }
                const bool miss = __builtin_amdgcn_ballot_w64(anym != 0u) != 0ull;   // wave-uniform
                saw_missing |= miss;
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) {
                    if (!act[rt]) continue;
                    xy[rt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(GA[rt], GB, xy[rt], 0, 0, 0);
                    if (miss) {
                        gm[rt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(GA[rt], MB, gm[rt], 0, 0, 0);
                        mg[rt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(MA[rt], GB, mg[rt], 0, 0, 0);
                        qm[rt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(QA[rt], MB, qm[rt], 0, 0, 0);
                        mq[rt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(MA[rt], QB, mq[rt], 0, 0, 0);
                        mm[rt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(MA[rt], MB, mm[rt], 0, 0, 0);
                    }
                }
            }
        }
        if (s + 1 < s1) ld_put<PACKED>(F, lds[(s + 1 - s0) & 1], s + 1, N, seg, lrow0, j0);   // (its last readers finished before the previous barrier)
        if (s + 2 < s1) ld_fetch<PACKED>(F, src, s + 2, seg, j0);
        __syncthreads();
    }
    if (s0 >= s1) return;

    const int64_t plane = (row1 - row0) * (int64_t)wmax;
    const int64_t j = c0 + 32 * wv + c;                   // the lane's column
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        if (!act[rt]) continue;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int64_t i = acc_row(i0 + 32 * rt, e, h);
            if (i >= row1 || j <= i) continue;
            if (j >= win_end[i - row0]) continue;
            const int64_t ix = (i - row0) * wmax + (j - i - 1);
            if (atomic) {
                atomicAdd(W + ix, xy[rt][e]);
                if (saw_missing) {
                    atomicAdd(W + plane + ix, gm[rt][e]); atomicAdd(W + 2 * plane + ix, mg[rt][e]); atomicAdd(W + 3 * plane + ix, qm[rt][e]);
                    atomicAdd(W + 4 * plane + ix, mq[rt][e]); atomicAdd(W + 5 * plane + ix, mm[rt][e]);
                }
            } else {
                W[ix] = xy[rt][e];
                if (saw_missing) {
                    W[plane + ix] = gm[rt][e]; W[2 * plane + ix] = mg[rt][e]; W[3 * plane + ix] = qm[rt][e];
                    W[4 * plane + ix] = mq[rt][e]; W[5 * plane + ix] = mm[rt][e];
                }
            }
        }
    }
}

void launch_ld(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t K, int64_t N, int64_t row0,
               int64_t row1, const int64_t* win_end, int wmax, int weff, int* W) {
    if (row1 <= row0 || weff <= 0) return;
    const int64_t nrb = ld_row_blocks(row1 - row0), nch = ld_col_chunks(weff), nst = ld_stages(N);
    const int64_t per = ld_stages_per_split(nrb * nch, nst), S = ld_splits(nrb * nch, nst);
    const dim3 grid((unsigned)(nrb * nch), (unsigned)S);
    const int atomic = S > 1 ? 1 : 0;
    if (packed) hipLaunchKernelGGL(k_ld<true>, grid, dim3(kLdThreads), 0, st, G, ldr, krows, K, N, row0, row1, win_end, wmax, weff, nrb, nst, per, atomic, W);
    else hipLaunchKernelGGL(k_ld<false>, grid, dim3(kLdThreads), 0, st, G, ldr, krows, K, N, row0, row1, win_end, wmax, weff, nrb, nst, per, atomic, W);
}

// Per kept row r of [row0, hi): stat[3 (r - row0)] = sum g', + 1 = sum g'^2, + 2 = missing calls over the N samples (one wave per row);
// *bad = the smallest original row index among those rows that hold a value outside {0, 1, 2, -127} (untouched when there is none).
template <bool PACKED>
__global__ __launch_bounds__(256) void k_ld_vec(const void* __restrict__ Gv, int64_t ldr, const int64_t* __restrict__ krows, int64_t N,
                                                int64_t row0, int64_t hi, unsigned* __restrict__ stat, unsigned long long* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int64_t r = row0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= hi) return;
    const int64_t orow = krows[r];
    const uint8_t* src = (const uint8_t*)Gv + orow * ldr;
    unsigned sx = 0, sq = 0, nm = 0, bd = 0;
    for (int64_t k = 16 * (int64_t)lane; k < N; k += 16 * 64) {
        uint4 v;
        if (PACKED) {
            const unsigned p = *reinterpret_cast<const unsigned*>(src + k / 4);
            v = make_uint4(unpack4(p & 0xffu), unpack4((p >> 8) & 0xffu), unpack4((p >> 16) & 0xffu), unpack4(p >> 24));
        } else v = *reinterpret_cast<const uint4*>(src + k);
        const int nvalid = N - k >= 16 ? 16 : (int)(N - k);
        const unsigned d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const unsigned a = d[w] & ld_tail_mask(w, nvalid);
            unsigned g, m, q;
            ld_ops(a, g, m, q);
            // valid bytes: 0, 1, 2 and 0x81.  A byte with bit 7 set must be exactly 0x81; the others must be below 3
            if ((a & (m * 0xffu)) != m * 0x81u || (g & 0xfcfcfcfcu) != 0u || (g & (g >> 1) & 0x01010101u) != 0u) bd = 1u;
            sx += __popc(g & 0x01010101u) + 2 * __popc(g & 0x02020202u);
            sq += __popc(q & 0x01010101u) + 4 * __popc(q & 0x04040404u);
            nm += __popc(m);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        sx += __shfl_xor(sx, o); sq += __shfl_xor(sq, o); nm += __shfl_xor(nm, o); bd |= __shfl_xor(bd, o);
    }
    if (lane == 0) {
        unsigned* o = stat + 3 * (r - row0);
        o[0] = sx; o[1] = sq; o[2] = nm;
        if (bd) atomicMin(bad, (unsigned long long)orow);
    }
}
void launch_ld_vec(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t N, int64_t row0, int64_t hi,
                   unsigned* stat, unsigned long long* bad) {
    if (hi <= row0) return;
    const dim3 grid((unsigned)((hi - row0 + 3) / 4));
    if (packed) hipLaunchKernelGGL(k_ld_vec<true>, grid, dim3(256), 0, st, G, ldr, krows, N, row0, hi, stat, bad);
    else hipLaunchKernelGGL(k_ld_vec<false>, grid, dim3(256), 0, st, G, ldr, krows, N, row0, hi, stat, bad);
}

// One wave per band row t and word of 64 slots: the six counts of the pair from the product planes and the per-row sums, r^2 in f64 on
// exact integers (all below 2^53; the three differences are exact, the two products and the division round once each):
//   n = N - miss_i - miss_j + mm,  sx = sum g'_i - g'm,  sy = sum g'_j - mg',  sxx = sum q_i - qm,  syy = sum q_j - mq,  sxy = g'g'
//   cov = n sxy - sx sy,  vx = n sxx - sx sx,  vy = n syy - sy sy,  r2 = (cov cov) / (vx vy)   (NaN when vx <= 0 or vy <= 0)
// Slots outside the row's window get 0 in r2, counts and above (any of which may be NULL).
__global__ __launch_bounds__(256) void k_ld_finish(const int* __restrict__ W, const unsigned* __restrict__ stat, int64_t N, int64_t row0,
                                                   int64_t rows, const int64_t* __restrict__ win_end, int wmax, double threshold,
                                                   double* __restrict__ r2, int* __restrict__ counts, unsigned long long* __restrict__ above) {
    const int lane = threadIdx.x & 63;
    const int64_t nwords = ld_above_words(wmax), nwb = (nwords + 3) / 4;
    const int64_t t = (int64_t)blockIdx.x / nwb;
    const int64_t wd = ((int64_t)blockIdx.x % nwb) * 4 + (threadIdx.x >> 6);
    if (wd >= nwords) return;
    const int64_t d = wd * 64 + lane, i = row0 + t, j = i + 1 + d;
    const bool slot = d < wmax, valid = slot && j < win_end[t];
    double v = 0.0;
    int cn[6] = {0, 0, 0, 0, 0, 0};
    if (valid) {
        const int64_t plane = rows * (int64_t)wmax, ix = t * wmax + d;
        const unsigned* si = stat + 3 * t;
        const unsigned* sj = stat + 3 * (j - row0);
        const int xy = W[ix], gm = W[plane + ix], mg = W[2 * plane + ix], qm = W[3 * plane + ix], mq = W[4 * plane + ix], mm = W[5 * plane + ix];
        cn[0] = (int)(N - si[2] - sj[2]) + mm;
        cn[1] = (int)si[0] - gm; cn[2] = (int)sj[0] - mg;
        cn[3] = (int)si[1] - qm; cn[4] = (int)sj[1] - mq;
        cn[5] = xy;
        const double n = cn[0], sx = cn[1], sy = cn[2], sxx = cn[3], syy = cn[4], sxy = cn[5];
        const double cov = n * sxy - sx * sy, vx = n * sxx - sx * sx, vy = n * syy - sy * sy;
        v = (vx <= 0.0 || vy <= 0.0) ? __builtin_nan("") : (cov * cov) / (vx * vy);
    }
    if (slot) {
        if (r2) r2[t * wmax + d] = v;
        if (counts) {
            int* o = counts + 6 * (t * wmax + d);
#pragma unroll
            for (int q = 0; q < 6; ++q) o[q] = cn[q];
        }
    }
    if (above) {
        const unsigned long long bits = __builtin_amdgcn_ballot_w64(valid && v > threshold);
        if (lane == 0) above[t * nwords + wd] = bits;
    }
}
void launch_ld_finish(hipStream_t st, const int* W, const unsigned* stat, int64_t N, int64_t row0, int64_t row1, const int64_t* win_end,
                      int wmax, double threshold, double* r2, int* counts, unsigned long long* above) {
    if (row1 <= row0) return;
    const dim3 grid((unsigned)((row1 - row0) * ((ld_above_words(wmax) + 3) / 4)));
    hipLaunchKernelGGL(k_ld_finish, grid, dim3(256), 0, st, W, stat, N, row0, row1 - row0, win_end, wmax, threshold, r2, counts, above);
}

// LD scores (gpca_ld_score, gpca_ld_score.cpp; include/gpca.h section a19): the planes of a band reduced to one sum per row, no pair
// leaving the device.  A counted pair (vx > 0, vy > 0, n > 2) is worth v = r2, or r2 - (1 - r2) / (n - 2) when unbiased, as the integer
// q = rint(v 2^40) (half to even), added to its row AND to its partner; every sum is an integer, so neither the tiling nor the order of
// the atomics moves a bit.
// Workgroup = a tile of kLdScoreRows band rows (first: t0) x kLdScoreSlots slots (first: d0).  Thread p owns the partner row
// t0 + d0 + 1 + p: in step lt it reads slot d0 + p - lt of row t0 + lt, so the threads of a step read consecutive slots of one row (the
// six plane reads are coalesced) while the partner's sum stays in the thread's registers over the steps -- the anti-diagonal is walked
// without a strided read and without an atomic.  The row's own sum is the step's sum over the threads: a wave reduction and one LDS
// atomic per wave.  Count and sum travel in one 64-bit word ((1 << kLdScoreCountShift) + q per pair).  At the end of the tile every
// touched target gets one 64-bit and one 32-bit global atomic.
// acc [span] i64 and partners [span] i32, zeroed by the caller; nstat = the rows stat holds from row0 (every valid partner lies below).
__device__ __forceinline__ long long ld_score_pair(const int* __restrict__ W, int64_t plane, int64_t ix, const unsigned* __restrict__ si,
                                                   const unsigned (&sj)[3], int64_t N, int unbiased) {
    // the six counts and r^2: a second copy of k_ld_finish's expression, kept in this file under the same compiler settings so that it
    // rounds as that kernel does (k_ld_finish itself is left as it is)
    const int xy = W[ix], gm = W[plane + ix], mg = W[2 * plane + ix], qm = W[3 * plane + ix], mq = W[4 * plane + ix], mm = W[5 * plane + ix];
    const int c0 = (int)(N - si[2] - sj[2]) + mm;
    const int c1 = (int)si[0] - gm, c2 = (int)sj[0] - mg, c3 = (int)si[1] - qm, c4 = (int)sj[1] - mq;
    const double n = c0, sx = c1, sy = c2, sxx = c3, syy = c4, sxy = xy;
    const double cov = n * sxy - sx * sy, vx = n * sxx - sx * sx, vy = n * syy - sy * sy;
    if (vx <= 0.0 || vy <= 0.0 || n <= 2.0) return 0;
    const double r2 = (cov * cov) / (vx * vy);
    {
#pragma clang fp contract(off)
        const double v = unbiased ? r2 - (1.0 - r2) / (n - 2.0) : r2;
        return (1ll << kLdScoreCountShift) + __double2ll_rn(v * 1099511627776.0);
    }
}
// (count, sum) of a packed word: the sum is the low kLdScoreCountShift bits, signed
__device__ __forceinline__ void ld_score_unpack(long long s, int& count, long long& sum) {
    const long long half = 1ll << (kLdScoreCountShift - 1);
    sum = ((s + half) & ((1ll << kLdScoreCountShift) - 1)) - half;
    count = (int)((s - sum) >> kLdScoreCountShift);
}
__global__ __launch_bounds__(kLdScoreThreads) void k_ld_score(const int* __restrict__ W, const unsigned* __restrict__ stat, int64_t N,
                                                              int64_t row0, int64_t rows, int64_t nstat, const int64_t* __restrict__ win_end,
                                                              int wmax, int64_t nrt, int unbiased, long long* __restrict__ acc,
                                                              int* __restrict__ partners) {
    __shared__ unsigned long long self[kLdScoreRows];
    const int p = threadIdx.x, lane = p & 63;
    const int64_t t0 = ((int64_t)blockIdx.x % nrt) * kLdScoreRows, d0 = ((int64_t)blockIdx.x / nrt) * kLdScoreSlots;
    if (p < kLdScoreRows) self[p] = 0ull;
    __syncthreads();
    const int64_t jr = t0 + d0 + 1 + p;                    // the thread's partner row, from row0
    const int64_t plane = rows * (int64_t)wmax;
    unsigned sj[3] = {0u, 0u, 0u};
    if (jr < nstat) { sj[0] = stat[3 * jr]; sj[1] = stat[3 * jr + 1]; sj[2] = stat[3 * jr + 2]; }
    const int nlt = rows - t0 < kLdScoreRows ? (int)(rows - t0) : kLdScoreRows;
    long long part = 0;
    for (int lt = 0; lt < nlt; ++lt) {
        const int64_t t = t0 + lt;
        const int dl = p - lt;
        const int64_t d = d0 + dl;
        const bool valid = dl >= 0 && dl < kLdScoreSlots && d < wmax && jr < nstat && row0 + jr < win_end[t];
        long long add = 0;
        if (valid) add = ld_score_pair(W, plane, t * wmax + d, stat + 3 * t, sj, N, unbiased);
        part += add;
        if (__builtin_amdgcn_ballot_w64(add != 0) != 0ull) {                 // wave-uniform
            long long s = add;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
            if (lane == 0) atomicAdd(&self[lt], (unsigned long long)s);
        }
    }
    __syncthreads();
    int cnt;
    long long sum;
    if (part != 0) {
        ld_score_unpack(part, cnt, sum);
        atomicAdd(reinterpret_cast<unsigned long long*>(acc) + jr, (unsigned long long)sum);
        atomicAdd(partners + jr, cnt);
    }
    if (p < nlt && self[p] != 0ull) {
        ld_score_unpack((long long)self[p], cnt, sum);
        atomicAdd(reinterpret_cast<unsigned long long*>(acc) + t0 + p, (unsigned long long)sum);
        atomicAdd(partners + t0 + p, cnt);
    }
}
void launch_ld_score(hipStream_t st, const int* W, const unsigned* stat, int64_t N, int64_t row0, int64_t row1, int64_t hi,
                     const int64_t* win_end, int wmax, int weff, int unbiased, long long* acc, int* partners) {
    if (row1 <= row0 || weff <= 0) return;
    const int64_t rows = row1 - row0, nrt = ld_score_row_tiles(rows);
    const dim3 grid((unsigned)ld_score_grid(rows, weff));
    hipLaunchKernelGGL(k_ld_score, grid, dim3(kLdScoreThreads), 0, st, W, stat, N, row0, rows, hi - row0, win_end, wmax, nrt, unbiased, acc, partners);
}

}  // namespace gpca
