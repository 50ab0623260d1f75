// Projection of genotypes onto a fitted model with missing calls mean-imputed (gpca_project, gpca_project.cpp).
//
//   score[n][c] = sum over model rows i with g[i][n] observed of (g[i][n] - mu_i) r_i W[i][c]
//               = tscale_a . sum_i g'[i][n] q(r o W)[i][c]  +  c_a[c]  -  tscale_b . sum_i m[i][n] q(b o W)[i][c]
// with g' = the call, 0 where missing; m = the missing indicator; b = -mu r (the engine's shift); c_a = b^T W.  The first two terms are
// what gpca_transform computes (the same digit planes, the same f64 combine); the third puts back, for every missing call, the b W that
// c_a charged it.  Both products come out of ONE read of the genotypes: every 32-row block is decoded once into the two int8 B-operands
// (g' and m), which meet two sets of digit planes.  A wave whose block holds no missing code skips the indicator MFMAs (wave-uniform
// ballot) and runs K2's work only.
//
// Register-only, in the style of gemm_i8_simple.hip.  A wave covers 64 samples (not K2's 128): two sides x two 32-sample tiles x
// four digit planes x 16 = 256 accumulator registers; with 128 samples it would be 512, the whole register file.
#include "syrk_tile.h"

namespace gpca {

// one 32-row block of the wave's ring: the lane's dword of each of its 16 rows, the row mask of the block, both sides' digit planes
struct PrjBuf { unsigned g[16]; unsigned rm; i32x4 a[kDigits]; i32x4 b[kDigits]; };

template <int ND, bool LAZYB>
__device__ __forceinline__ void prj_load(PrjBuf& B, __amdgpu_buffer_rsrc_t rg, uint32_t gvo, uint32_t row_off, uint32_t ldr,
                                         const uint32_t* __restrict__ rmask, int64_t blk,
                                         __amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rb, uint32_t tvo, uint32_t toff) {
#pragma unroll
    for (int i = 0; i < 16; ++i) B.g[i] = (unsigned)__builtin_amdgcn_raw_buffer_load_b32(rg, gvo, row_off + (uint32_t)i * ldr, 0);
    B.rm = rmask[blk];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        B.a[d] = __builtin_amdgcn_raw_buffer_load_b128(ra, tvo, toff + d * 1024, 0);
        if (!LAZYB) B.b[d] = __builtin_amdgcn_raw_buffer_load_b128(rb, tvo, toff + d * 1024, 0);
    }
}

// The block's two operands per 32-sample tile t (sample n0 + 2c + t, rows 16h .. 16h + 15 as 16 k-contiguous bytes), the missing count
// of the lane's two samples over model rows, and the invalid-dosage bits of model rows (int8 rows only: 2-bit codes cannot be invalid).
// LAZYB: the indicator planes are not in the ring; a block with a missing code loads them here (from L2, behind the ballot)
template <bool PACKED, int ND, bool LAZYB>
__device__ __forceinline__ void prj_block(const PrjBuf& B, unsigned sh, int h, i32x16 (&acc_a)[2][kDigits], i32x16 (&acc_b)[2][kDigits],
                                          unsigned (&cnt)[2], unsigned& bad, bool& any_missing,
                                          __amdgpu_buffer_rsrc_t rb, uint32_t tvo, uint32_t toff) {
    unsigned p[16];   // byte 0: sample n0 + 2c, byte 1: sample n0 + 2c + 1 (int8 form; 2-bit codes keep their values 0..3)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (PACKED) { const unsigned nib = (B.g[i] >> sh) & 0xfu; p[i] = (nib & 3u) | ((nib & 0xcu) << 6); }
        else p[i] = (B.g[i] >> sh) & 0xffffu;
    }
    const unsigned mask16 = (B.rm >> (16 * h)) & 0xffffu;
    i32x4 og[2], om[2];
    unsigned mm[4], anym = 0u;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const unsigned x = p[4 * w] | (p[4 * w + 1] << 16), y = p[4 * w + 2] | (p[4 * w + 3] << 16);
        mm[w] = kept_bytes(mask16, w);   // byte q = 1: row 4w + q is a model row
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const unsigned v = (unsigned)permb((int)y, (int)x, t ? 0x07050301u : 0x06040200u);   // rows 4w .. 4w + 3 of sample t
            unsigned m, g;
            if (PACKED) { m = v & (v >> 1) & 0x01010101u; g = v & ~(m * 3u); }            // code 3 = missing
            else {
                m = (v >> 7) & 0x01010101u;                                                 // -127 = missing (any negative byte is at least not a dosage)
                g = v & ~(m * 0xffu);
                const unsigned lo = v & 0x7f7f7f7fu;
                const unsigned b1 = (lo + 0x7d7d7d7du) & 0x80808080u;                       // low 7 bits >= 3
                const unsigned b2 = ((lo ^ 0x01010101u) + 0x7f7f7f7fu) & v & 0x80808080u;  // sign set and not -127
                bad |= (b1 | b2) & (mm[w] << 7);
            }
            og[t][w] = (int)g; om[t][w] = (int)m; anym |= m;
        }
    }
#pragma unroll
    for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc_a[t][d] = __builtin_amdgcn_mfma_i32_32x32x32_i8(B.a[d], og[t], acc_a[t][d], 0, 0, 0);
    if (__builtin_amdgcn_ballot_w64(anym != 0u) != 0ull) {     // wave-uniform: the block holds a missing code somewhere
        any_missing = true;
        i32x4 pb[kDigits];
#pragma unroll
        for (int d = 0; d < ND; ++d) pb[d] = LAZYB ? __builtin_amdgcn_raw_buffer_load_b128(rb, tvo, toff + d * 1024, 0) : B.b[d];
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
            for (int t = 0; t < 2; ++t) acc_b[t][d] = __builtin_amdgcn_mfma_i32_32x32x32_i8(pb[d], om[t], acc_b[t][d], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int w = 0; w < 4; ++w) cnt[t] += (unsigned)__builtin_popcount((unsigned)om[t][w] & mm[w]);
    }
}

// Ypa / Ypb [W][Npad][32]: the wave chunk's exact integer sums of both sides (digits combined in f64, as K2 writes them); cnt [Npad]:
// missing calls in model rows, added atomically (exact, any order); bad: bit 0 set when a model row holds a value outside
// {0, 1, 2, -127}.  Grid = ngroups x W workgroups; wave = 64 samples x rows [m_begin, m_end) (a multiple of 128).
template <bool PACKED, int ND, bool LAZYB>
__global__ __launch_bounds__(256, 1) void k_project(const void* __restrict__ G, int64_t ldr, int64_t Mpad, int64_t Npad,
                                                     const int8_t* __restrict__ Ta, const int8_t* __restrict__ Tb,
                                                     const uint32_t* __restrict__ rmask, double* __restrict__ Ypa, double* __restrict__ Ypb,
                                                     unsigned* __restrict__ cnt_out, unsigned* __restrict__ bad_out,
                                                     int64_t ngroups, int64_t rows_per_wave) {
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int64_t ngroup = blockIdx.x % ngroups;
    const int64_t wchunk = blockIdx.x / ngroups;
    const int64_t n0 = (ngroup * 4 + wv) * 64;
    if (n0 >= Npad) return;
    const int64_t m_begin = wchunk * rows_per_wave;
    if (m_begin >= Mpad) return;
    const int64_t m_end = (m_begin + rows_per_wave < Mpad) ? m_begin + rows_per_wave : Mpad;
    const int64_t kblocks = (m_end - m_begin) >> 5;   // multiple of 4

    i32x16 acc_a[2][kDigits], acc_b[2][kDigits];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int d = 0; d < kDigits; ++d)
#pragma unroll
            for (int e = 0; e < 16; ++e) { acc_a[t][d][e] = 0; acc_b[t][d][e] = 0; }
    unsigned cnt[2] = {0u, 0u}, bad = 0u;
    bool any_missing = false;

    // the lane's samples n0 + 2c, n0 + 2c + 1: int8 rows -> bytes 2c, 2c + 1 of the wave's 64; 2-bit rows -> nibble c of its 16 bytes
    const uint32_t gvo = PACKED ? (uint32_t)(16 * h * ldr + 4 * (c >> 3)) : (uint32_t)(16 * h * ldr + 4 * (c >> 1));
    const unsigned sh = PACKED ? 8u * (unsigned)((c >> 1) & 3) + 4u * (unsigned)(c & 1) : 16u * (unsigned)(c & 1);
    const uint32_t tvo = (uint32_t)(lane * 16);
    constexpr uint32_t TKB = kDigits * 1024;
    const uint8_t* gp = (const uint8_t*)G + m_begin * ldr + (PACKED ? n0 / 4 : n0);
    const int8_t* ta = Ta + (m_begin >> 5) * TKB;
    const int8_t* tb = Tb + (m_begin >> 5) * TKB;
    const uint32_t* rm = rmask + (m_begin >> 5);
    PrjBuf B0, B1, B2, B3;
    {
        const __amdgpu_buffer_rsrc_t rg0 = make_rsrc8(gp), ra0 = make_rsrc8(ta), rb0 = make_rsrc8(tb);
        prj_load<ND, LAZYB>(B0, rg0, gvo, 0u, (uint32_t)ldr, rm, 0, ra0, rb0, tvo, 0u);
        prj_load<ND, LAZYB>(B1, rg0, gvo, 32u * (uint32_t)ldr, (uint32_t)ldr, rm, 1, ra0, rb0, tvo, TKB);
        prj_load<ND, LAZYB>(B2, rg0, gvo, 64u * (uint32_t)ldr, (uint32_t)ldr, rm, 2, ra0, rb0, tvo, 2 * TKB);
    }
    // 4-stage register ring over 32-row blocks: 3 blocks in flight per wave (the last trip reloads blocks it already has: in bounds)
    for (int64_t kb = 0; kb < kblocks; kb += 4) {
        const __amdgpu_buffer_rsrc_t rg = make_rsrc8(gp + kb * 32 * ldr);   // re-based every trip: offsets stay < 256 * ldr
        const __amdgpu_buffer_rsrc_t ra = make_rsrc8(ta + kb * TKB), rb = make_rsrc8(tb + kb * TKB);
        const uint32_t more = (kb + 4 < kblocks) ? 1u : 0u;
        const uint32_t L32 = 32u * (uint32_t)ldr;
        const uint32_t* rmk = rm + kb;
        prj_load<ND, LAZYB>(B3, rg, gvo, 3u * L32, (uint32_t)ldr, rmk, 3, ra, rb, tvo, 3 * TKB);
        prj_block<PACKED, ND, LAZYB>(B0, sh, h, acc_a, acc_b, cnt, bad, any_missing, rb, tvo, 0);
        prj_load<ND, LAZYB>(B0, rg, gvo, 4u * L32 * more, (uint32_t)ldr, rmk, 4 * more, ra, rb, tvo, 4 * TKB * more);
        prj_block<PACKED, ND, LAZYB>(B1, sh, h, acc_a, acc_b, cnt, bad, any_missing, rb, tvo, TKB);
        prj_load<ND, LAZYB>(B1, rg, gvo, (4u * more + 1u) * L32, (uint32_t)ldr, rmk, 4 * more + 1, ra, rb, tvo, (4 * more + 1) * TKB);
        prj_block<PACKED, ND, LAZYB>(B2, sh, h, acc_a, acc_b, cnt, bad, any_missing, rb, tvo, 2 * TKB);
        prj_load<ND, LAZYB>(B2, rg, gvo, (4u * more + 2u) * L32, (uint32_t)ldr, rmk, 4 * more + 2, ra, rb, tvo, (4 * more + 2) * TKB);
        prj_block<PACKED, ND, LAZYB>(B3, sh, h, acc_a, acc_b, cnt, bad, any_missing, rb, tvo, 3 * TKB);
    }
    // D[j][col]: j = acc_row(0, reg, h), col = c -> sample n0 + 2c + t.  Exact integers as f64.
    double* ya = Ypa + (wchunk * Npad) * 32;
    double* yb = Ypb + (wchunk * Npad) * 32;
    constexpr int BITS = ND == 3 ? 8 : 7;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int64_t n = n0 + 2 * c + t;
#pragma unroll
        for (int e = 0; e < 16; e += 2) {
            const int j = acc_row(0, e, h);
            double2 o;
            o.x = combine_digits<BITS>(acc_a[t], e); o.y = combine_digits<BITS>(acc_a[t], e + 1);
            *reinterpret_cast<double2*>(ya + n * 32 + j) = o;
            o.x = combine_digits<BITS>(acc_b[t], e); o.y = combine_digits<BITS>(acc_b[t], e + 1);
            *reinterpret_cast<double2*>(yb + n * 32 + j) = o;
        }
    }
    if (any_missing && cnt_out) {      // (NULL: another launch of the call counts these samples)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const unsigned tot = cnt[t] + (unsigned)__shfl_xor((int)cnt[t], 32);   // rows 0-15 and 16-31 of every block
            if (h == 0 && tot) atomicAdd(cnt_out + n0 + 2 * c + t, tot);
        }
    }
    if (bad) atomicOr(bad_out, 1u);
}

// (the plan: prj_plan, plan_math.h)

void launch_project(hipStream_t st, const void* G, int packed, int64_t ldr, int64_t Mpad, int64_t Npad, const int8_t* Ta, const int8_t* Tb,
                    const uint32_t* rmask, double* Ypa, double* Ypb, unsigned* cnt, unsigned* bad, const PrjPlan& plan, int nd, int lazy_b) {
    const dim3 grid((unsigned)plan.grid), blk(256);
#define PRJ_LAUNCH(P, D, Z) hipLaunchKernelGGL((k_project<P, D, Z>), grid, blk, 0, st, G, ldr, Mpad, Npad, Ta, Tb, rmask, Ypa, Ypb, cnt, bad, plan.ngroups, plan.rows_per_wave)
#define PRJ_LAUNCH_Z(P, D) do { if (lazy_b) PRJ_LAUNCH(P, D, true); else PRJ_LAUNCH(P, D, false); } while (0)
    if (packed) { if (nd == 3) PRJ_LAUNCH_Z(true, 3); else PRJ_LAUNCH_Z(true, kDigits); }
    else { if (nd == 3) PRJ_LAUNCH_Z(false, 3); else PRJ_LAUNCH_Z(false, kDigits); }
#undef PRJ_LAUNCH_Z
#undef PRJ_LAUNCH
}

// Y[n][j] = fma(-tscale_b[j], Yint_b[n][j], Y[n][j]) for j < 32 of one half (pitch ldy); an exact zero correction leaves Y's bits alone.
// A sample with no observed call in the model rows (n_model == cnt[n]) scores exactly 0: a sum over no rows.
__global__ __launch_bounds__(256) void k_project_correct(const double* __restrict__ Yb, int64_t N, const double* __restrict__ tscale_b,
                                                         const unsigned* __restrict__ cnt, int64_t n_model, double* __restrict__ Y, int64_t ldy) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= N * 32) return;
    const int j = (int)(e & 31);
    double* y = Y + (e >> 5) * ldy + j;
    *y = (int64_t)cnt[e >> 5] == n_model ? 0.0 : fma(-tscale_b[j], Yb[e], *y);
}
void launch_project_correct(hipStream_t st, const double* Yint_b, int64_t N, const double* tscale_b, const unsigned* cnt, int64_t n_model,
                            double* Y, int64_t ldy) {
    hipLaunchKernelGGL(k_project_correct, dim3((unsigned)((N * 32 + 255) / 256)), dim3(256), 0, st, Yint_b, N, tscale_b, cnt, n_model, Y, ldy);
}
// out[j] = max(out[j], max_i |X[i][j]|) for j < L (a multiple of 32) as the bits of a non-negative double (their order is the values')
__global__ __launch_bounds__(256) void k_project_colmax(const float* __restrict__ X, int64_t rows, int L, unsigned long long* __restrict__ out) {
    __shared__ double red[256];
    const int cc = threadIdx.x & 31, rg = threadIdx.x >> 5;
    for (int j0 = 0; j0 < L; j0 += 32) {
        double a = 0.0;
        for (int64_t i = (int64_t)blockIdx.x * 8 + rg; i < rows; i += (int64_t)gridDim.x * 8) {
            const double v = fabs((double)X[i * L + j0 + cc]);
            a = v > a ? v : a;
        }
        red[threadIdx.x] = a;
        __syncthreads();
        if (rg == 0) {
            for (int g = 1; g < 8; ++g) { const double v = red[g * 32 + cc]; a = v > a ? v : a; }
            if (a > 0.0) atomicMax(out + j0 + cc, (unsigned long long)__double_as_longlong(a));
        }
        __syncthreads();
    }
}
void launch_project_colmax(hipStream_t st, const float* X, int64_t rows, int L, unsigned long long* out) {
    const int64_t g = std::min<int64_t>(1024, (rows + 7) / 8);
    hipLaunchKernelGGL(k_project_colmax, dim3((unsigned)std::max<int64_t>(g, 1)), dim3(256), 0, st, X, rows, L, out);
}
// used[n] = n_model - cnt[n] as f64 (the ranks' counts are summed by the same exchange as the scores)
__global__ __launch_bounds__(256) void k_project_used(const unsigned* __restrict__ cnt, int64_t N, double n_model, double* __restrict__ used) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n < N) used[n] = n_model - (double)cnt[n];
}
void launch_project_used(hipStream_t st, const unsigned* cnt, int64_t N, double n_model, double* used) {
    hipLaunchKernelGGL(k_project_used, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, cnt, N, n_model, used);
}

}  // namespace gpca
