// The two tall-skinny products of the randomized PCA on v_mfma_f32_32x32x2_f32 (exact f32 FMA chains).
//
//   K1  k_gq_f32 :  T[M][L]  = r o (G Q) + b s^T          contraction over samples  (2*M*N*l flop / M*N bytes)
//   K2  k_gtt_f32:  Y^T tiles = (r o T)^T G               contraction over SNPs     (2*M*N*l flop / M*N bytes)
//
// Arithmetic intensity 2*l = 60 flop/B >> the gfx950 ridge (~20 flop/B): MFMA-fp32 bound.  Measured facts the
// structure is built on (scripts/kbench/kbench_gtt.hip, MI355X):
//   * a bare 32x32x2 f32 MFMA loop runs 154 TF (98 %); ANY VALU instruction issued between the MFMAs costs
//     MFMA time (f32 MFMA shares the f32 lanes): 1 dependent v_cvt_f32_ubyte per MFMA -> 115-133 TF.
//     => the int8 dosages are converted in a block before the MFMA block, two per instruction, with
//        v_cvt_pk_f32_fp8: bytes 0/1/2 read as fp8-e4m3 subnormals are exactly g * 2^-9; the 2^9 is multiplied
//        back in the epilogue (exact), so results equal the plain int->float path bit for bit.
//   * one wave per SIMD with all loads of the next step in flight behind the current step's 64-128 MFMAs beats
//     two waves per SIMD; loads use buffer descriptors with SGPR offsets (no per-lane address VALU), the
//     skinny operand is stored blocked so that a lane fetches its 8/16 k-steps with 16-byte loads, and the
//     double buffer is a branch-free 2x unrolled swap (no v_mov).
//   Result: 140 TF (89 % of the 157 TF MFMA-f32 peak) on the padded shape.
//
// G is read straight from HBM into registers: each byte feeds exactly one MFMA, so LDS staging would add
// traffic without reuse.  Both kernels also run on 2-bit resident genotypes (GPCA_STORE_2BIT, template PACKED): the codes
// are spread to one byte each in the conversion block (4 shift/mask per 16 samples in K1, a 2-step bit spread per 4 samples
// in K2) and then take the same fp8 path -- the same f32 FMA chains, so the results equal the int8-resident run bit for bit,
// at a quarter of the HBM bytes (north_star's 10M SNPs x 100k samples = 250 GB fit one MI355X).  Rows of G/T are zero-padded to a multiple of 128 and samples to a multiple of 256,
// so the main loops carry no predicates.
//
// Blocked layouts (written by the producing kernels, see blocked_* helpers in kernels.h):
//   Qb  [chunk = s/32][lt][lane = 32*h + c][u = 0..15]   = Q[32*chunk + 16*h + u][32*lt + c]
//   Tb  [group = i/16][lt][lane = 32*h + c][u = 0..7]    = T'[16*group + 2*u + h][32*lt + c]
#include "kernels.h"

namespace gpca {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

#define GPCA_RSRC_FLAGS 0x00020000
constexpr float kFp8Unscale = 512.0f;   // 2^9: bytes {0,1,2} as fp8-e4m3 subnormals are g * 2^-9

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7fffffff, GPCA_RSRC_FLAGS);
}

// ------------------------------------------------------------------------------------------------
// K1.  MFMA A = 32 SNP rows x 2 samples (lane l: row l&31, k = l>>5), B = 2 samples x 32 columns of Q.
// The grid is a fixed set of resident waves (GqPlan), one per SIMD; wave w owns a contiguous, balanced range
// of 32-row units and processes it in groups of R = 8/4/2/1 row tiles.  Per group the wave walks the samples
// in chunks of 32: lane (c, h) loads the 16 bytes [s0+16h, s0+16h+16) of row c of each tile; byte u is the A
// operand of k-step u; the lane's 16 Q values of the chunk (one 64-byte run of Qb) are the B operands.
// ------------------------------------------------------------------------------------------------
// (the plan: gq_plan, plan_math.h)

// One 128-sample super-chunk of a group's R row tiles.  int8 rows: the four 32-byte pieces of a row's 128-byte line are
// requested back to back by the same lanes (one L1 miss + three hits); requested one piece per 32-sample chunk -- 8 192
// MFMA cycles apart -- the lines were evicted from L2 in between and came in again from the fabric (FETCH_SIZE 2.25 x the
// matrix).  Packed rows (2-bit dosage codes, GPCA_STORE_2BIT): 32 bytes per row per super-chunk, both lane halves load the
// same 16 bytes (64 samples) and take their own dword.
template <int R, bool PACKED>
struct GqG { i32x4 g[PACKED ? 2 : 4][R]; };
template <int LT>
struct GqQ { i32x4 q0[LT], q1[LT], q2[LT], q3[LT]; };

template <int R, bool PACKED>
__device__ __forceinline__ void gq_load_g(GqG<R, PACKED>& b, __amdgpu_buffer_rsrc_t rg, const uint32_t (&gvo)[R], uint32_t s0) {
#pragma unroll
    for (int t = 0; t < R; ++t)
#pragma unroll
        for (int j = 0; j < (PACKED ? 2 : 4); ++j)
            b.g[j][t] = __builtin_amdgcn_raw_buffer_load_b128(rg, gvo[t], PACKED ? (s0 >> 2) + 16u * j : s0 + 32u * j, 0);
}
template <int LT>
__device__ __forceinline__ void gq_load_q(GqQ<LT>& b, __amdgpu_buffer_rsrc_t rq, uint32_t qvo, uint32_t qoff) {
#pragma unroll
    for (int lt = 0; lt < LT; ++lt) {
        b.q0[lt] = __builtin_amdgcn_raw_buffer_load_b128(rq, qvo, qoff + lt * 4096, 0);
        b.q1[lt] = __builtin_amdgcn_raw_buffer_load_b128(rq, qvo + 16, qoff + lt * 4096, 0);
        b.q2[lt] = __builtin_amdgcn_raw_buffer_load_b128(rq, qvo + 32, qoff + lt * 4096, 0);
        b.q3[lt] = __builtin_amdgcn_raw_buffer_load_b128(rq, qvo + 48, qoff + lt * 4096, 0);
    }
}

// chunk J (0..3) of the super-chunk held in b: 16 k-steps of 32x32x2 MFMAs per tile and column block
template <int R, int LT, bool PACKED, int J>
__device__ __forceinline__ void gq_compute(const GqG<R, PACKED>& b, const GqQ<LT>& q, f32x16 (&acc)[R][LT], int h) {
    float av[R][16];
#pragma unroll
    for (int t = 0; t < R; ++t) {
        if (PACKED) {
            // the lane's 16 samples of this chunk = one dword of codes: field s at bits 2s.  (w >> 2j) & 0x03030303 leaves the
            // codes of samples j, 4+j, 8+j, 12+j in bytes 0..3 -- as fp8-e4m3 subnormals exactly g * 2^-9
            const int lo_ = b.g[J >> 1][t][2 * (J & 1)], hi_ = b.g[J >> 1][t][2 * (J & 1) + 1];
            const unsigned w = (unsigned)(h ? hi_ : lo_);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = (int)((w >> (2 * j)) & 0x03030303u);
                const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(x, false);
                const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(x, true);
                av[t][j] = lo[0]; av[t][4 + j] = lo[1]; av[t][8 + j] = hi[0]; av[t][12 + j] = hi[1];
            }
        } else {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(b.g[PACKED ? 0 : J][t][v], false);
                const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(b.g[PACKED ? 0 : J][t][v], true);
                av[t][4 * v + 0] = lo[0]; av[t][4 * v + 1] = lo[1]; av[t][4 * v + 2] = hi[0]; av[t][4 * v + 3] = hi[1];
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 16; ++u)
#pragma unroll
        for (int lt = 0; lt < LT; ++lt) {
            // (element picked with plain constant subscripts: `v[u & 3]` made hipcc 7.2 narrow the 16-byte loads to
            //  one dword and feed element 0 to all four k-steps)
            const float qv = __builtin_bit_cast(float, u < 4 ? q.q0[lt][u] : u < 8 ? q.q1[lt][u - 4] : u < 12 ? q.q2[lt][u - 8] : q.q3[lt][u - 12]);
#pragma unroll
            for (int t = 0; t < R; ++t) acc[t][lt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t][u], qv, acc[t][lt], 0, 0, 0);
        }
}

template <int R, int LT, bool PACKED>
__device__ __forceinline__ void gq_group(const void* __restrict__ Gv, int64_t ldr, int64_t nsuper,
                                         const float* __restrict__ Qb, const float* __restrict__ rv,
                                         const float* __restrict__ bv, const float (&sj)[LT], float* __restrict__ Tout,
                                         float* __restrict__ Tb, float (&csum)[LT], int64_t row0, int c, int h, int lane) {
    constexpr int L = 32 * LT;
    const __amdgpu_buffer_rsrc_t rg = make_rsrc(static_cast<const char*>(Gv) + row0 * ldr);
    uint32_t gvo[R];
#pragma unroll
    for (int t = 0; t < R; ++t) gvo[t] = (uint32_t)((32 * t + c) * ldr + (PACKED ? 0 : 16 * h));
    const uint32_t qvo = (uint32_t)(lane * 64);
    constexpr uint32_t QCH = LT * 4096;   // bytes of Qb per 32-sample chunk

    f32x16 acc[R][LT];
#pragma unroll
    for (int t = 0; t < R; ++t)
#pragma unroll
        for (int lt = 0; lt < LT; ++lt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[t][lt][e] = 0.f;

    GqG<R, PACKED> GA, GB;
    GqQ<LT> QA, QB;
    gq_load_g<R, PACKED>(GA, rg, gvo, 0u);
    gq_load_q<LT>(QA, make_rsrc(Qb), qvo, 0u);
    // super-chunks (128 samples = 4 chunks) are processed in pairs; nsuper is even (samples padded to a multiple of 256).
    // Q rides one chunk ahead (QA / QB alternate), G one super-chunk ahead (GA / GB alternate).
#define GQF_STEP(GCUR, J, QCUR, QNXT, QOFF)                       \
    gq_load_q<LT>(QNXT, rq, qvo, (QOFF));                          \
    __builtin_amdgcn_sched_barrier(0);                             \
    gq_compute<R, LT, PACKED, J>(GCUR, QCUR, acc, h);              \
    __builtin_amdgcn_sched_barrier(0);
    for (int64_t sc = 0; sc < nsuper; sc += 2) {
        const __amdgpu_buffer_rsrc_t rq = make_rsrc(reinterpret_cast<const char*>(Qb) + sc * 4 * QCH);
        const uint32_t s0 = (uint32_t)(sc * 128);
        const uint32_t more = (sc + 2 < nsuper) ? 1u : 0u;   // the last trip prefetches its own first data (unused)
        gq_load_g<R, PACKED>(GB, rg, gvo, s0 + 128u);
        GQF_STEP(GA, 0, QA, QB, 1 * QCH) GQF_STEP(GA, 1, QB, QA, 2 * QCH) GQF_STEP(GA, 2, QA, QB, 3 * QCH) GQF_STEP(GA, 3, QB, QA, 4 * QCH)
        gq_load_g<R, PACKED>(GA, rg, gvo, s0 + 256u * more);
        GQF_STEP(GB, 0, QA, QB, 5 * QCH) GQF_STEP(GB, 1, QB, QA, 6 * QCH) GQF_STEP(GB, 2, QA, QB, 7 * QCH) GQF_STEP(GB, 3, QB, QA, 8 * QCH * more)
    }
#undef GQF_STEP

    // epilogue: D[row][col]: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5).  Pad rows have r = b = 0.
#pragma unroll
    for (int t = 0; t < R; ++t) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int64_t row = acc_row(row0 + 32 * t, e, h);
            const float ri = rv[row], bi = bv[row];
#pragma unroll
            for (int lt = 0; lt < LT; ++lt) {
                const float tv = ri * (acc[t][lt][e] * kFp8Unscale) + bi * sj[lt];
                if (Tb) {   // power iteration: T' = r o T in the blocked layout K2 reads, plus c = b^T T
                    csum[lt] += bi * tv;
                    Tb[blocked_t_index(row, 32 * lt + c, LT)] = ri * tv;
                } else {
                    Tout[row * L + 32 * lt + c] = tv;
                }
            }
        }
    }
}

template <int LT, bool PACKED>
__global__ __launch_bounds__(256, 1) void k_gq_f32(const void* __restrict__ G, int64_t ldr, int64_t units,
                                                    int64_t nsuper, const float* __restrict__ Qb,
                                                    const float* __restrict__ rv, const float* __restrict__ bv,
                                                    const float* __restrict__ sv, float* __restrict__ Tout,
                                                    float* __restrict__ Tb, float* __restrict__ cpart) {
    constexpr int L = 32 * LT;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int64_t wave = (int64_t)blockIdx.x * 4 + wv;
    const int64_t waves = (int64_t)gridDim.x * 4;
    int64_t u = (units * wave) / waves;                 // balanced contiguous ranges of 32-row units
    const int64_t u_end = (units * (wave + 1)) / waves;

    float csum[LT], sj[LT];
#pragma unroll
    for (int lt = 0; lt < LT; ++lt) { csum[lt] = 0.f; sj[lt] = sv[32 * lt + c]; }
    for (; u + 4 <= u_end; u += 4) gq_group<4, LT, PACKED>(G, ldr, nsuper, Qb, rv, bv, sj, Tout, Tb, csum, u * 32, c, h, lane);
    if (u + 2 <= u_end) { gq_group<2, LT, PACKED>(G, ldr, nsuper, Qb, rv, bv, sj, Tout, Tb, csum, u * 32, c, h, lane); u += 2; }
    if (u + 1 <= u_end) { gq_group<1, LT, PACKED>(G, ldr, nsuper, Qb, rv, bv, sj, Tout, Tb, csum, u * 32, c, h, lane); u += 1; }
#pragma unroll
    for (int lt = 0; lt < LT; ++lt) {
        const float o = csum[lt] + __shfl_xor(csum[lt], 32);
        if (h == 0) cpart[wave * L + 32 * lt + c] = o;
    }
}

// G: int8 rows of pitch ldr (packed = 0) or 2-bit dosage codes of pitch ldr bytes (packed = 1); Npad = padded sample count
void launch_gq_f32(hipStream_t st, const void* G, int packed, int64_t ldr, const GqPlan& plan, int64_t Npad, const float* Qb, int L,
                   const float* r, const float* b, const float* s, float* Tout, float* Tb, float* cpart) {
    const dim3 grid((unsigned)(plan.waves / 4)), blk(256);
    const int64_t nsuper = Npad / 128;   // even: Npad is a multiple of 256
#define GPCA_GQF(LTV, PK) hipLaunchKernelGGL((k_gq_f32<LTV, PK>), grid, blk, 0, st, G, ldr, plan.units, nsuper, Qb, r, b, s, Tout, Tb, cpart)
    if (L == 32) { if (packed) GPCA_GQF(1, true); else GPCA_GQF(1, false); }
    else { if (packed) GPCA_GQF(2, true); else GPCA_GQF(2, false); }
#undef GPCA_GQF
}

// ------------------------------------------------------------------------------------------------
// K2.  D = Y^T tile: A = T'^T (32 columns j x 2 SNPs), B = G (2 SNPs x 32 samples).  Lane (c, h) loads the
// 8 bytes [n0+8c, n0+8c+8) of SNP row m+2u+h: one wave-load = 2 rows x 256 contiguous bytes.  Byte t feeds
// accumulator tile t, whose MFMA column c is sample n0 + 8c + t.  A wave owns one 256-sample block and a
// contiguous range of SNP rows (groups of 16 = 8 k-steps; the lane's 8 T' values of a group are one 32-byte
// run of Tb); partial Y^T tiles go to Ypart and are summed in f64 by k_reduce_y (deterministic, no atomics).
// ------------------------------------------------------------------------------------------------
// (the plan: gtt_plan, plan_math.h)

template <int LT>
struct GttBuf { i32x2 g[8]; i32x4 t0[LT], t1[LT]; };

// PACKED: the lane's 8 samples are 16 bits of the row; lanes 2j and 2j+1 load the same dword and take their own half
template <int LT, bool PACKED>
__device__ __forceinline__ void gtt_load(GttBuf<LT>& b, __amdgpu_buffer_rsrc_t rg, uint32_t gvo, uint32_t row_off,
                                         uint32_t ldg, __amdgpu_buffer_rsrc_t rt, uint32_t tvo, uint32_t toff) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        if (PACKED) b.g[u][0] = __builtin_amdgcn_raw_buffer_load_b32(rg, gvo, row_off + (uint32_t)(2 * u) * ldg, 0);
        else b.g[u] = __builtin_amdgcn_raw_buffer_load_b64(rg, gvo, row_off + (uint32_t)(2 * u) * ldg, 0);
    }
#pragma unroll
    for (int lt = 0; lt < LT; ++lt) {
        b.t0[lt] = __builtin_amdgcn_raw_buffer_load_b128(rt, tvo, toff + lt * 2048, 0);
        b.t1[lt] = __builtin_amdgcn_raw_buffer_load_b128(rt, tvo + 16, toff + lt * 2048, 0);
    }
}

// one byte of 2-bit codes (4 samples) -> 4 bytes, one code each
__device__ __forceinline__ int spread_codes(unsigned t) {
    t = (t | (t << 12)) & 0x000F000Fu;
    t = (t | (t << 6)) & 0x03030303u;
    return (int)t;
}

template <int LT, bool PACKED>
__device__ __forceinline__ void gtt_compute(const GttBuf<LT>& b, f32x16 (&acc)[8][LT], unsigned hsh) {
    float bv[8][8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        int g0, g1;
        if (PACKED) {
            const unsigned w = ((unsigned)b.g[u][0] >> hsh) & 0xffffu;     // this lane's 8 samples
            g0 = spread_codes(w & 0xffu); g1 = spread_codes(w >> 8);
        } else { g0 = b.g[u][0]; g1 = b.g[u][1]; }
        const f32x2 p0 = __builtin_amdgcn_cvt_pk_f32_fp8(g0, false), p1 = __builtin_amdgcn_cvt_pk_f32_fp8(g0, true);
        const f32x2 p2 = __builtin_amdgcn_cvt_pk_f32_fp8(g1, false), p3 = __builtin_amdgcn_cvt_pk_f32_fp8(g1, true);
        bv[u][0] = p0[0]; bv[u][1] = p0[1]; bv[u][2] = p1[0]; bv[u][3] = p1[1];
        bv[u][4] = p2[0]; bv[u][5] = p2[1]; bv[u][6] = p3[0]; bv[u][7] = p3[1];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int lt = 0; lt < LT; ++lt) {
            const float ta = __builtin_bit_cast(float, u < 4 ? b.t0[lt][u] : b.t1[lt][u - 4]);
#pragma unroll
            for (int t = 0; t < 8; ++t) acc[t][lt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ta, bv[u][t], acc[t][lt], 0, 0, 0);
        }
}

template <int LT, bool PACKED>
__global__ __launch_bounds__(256, 1) void k_gtt_f32(const uint8_t* __restrict__ G, int64_t ldg, int64_t Mpad,
                                                     int64_t Npad, const float* __restrict__ Tb,
                                                     float* __restrict__ Ypart, int64_t ngroups, int64_t rows_per_wave) {
    constexpr int L = 32 * LT;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    // (an XCD-aware block -> (row chunk, n-group) remap was measured: no gain -- the skinny operand is already
    //  L2/MALL-served -- and its padded grid broke the all-blocks-resident property, so the plain mapping stays)
    const int64_t ngroup = blockIdx.x % ngroups;
    const int64_t wchunk = blockIdx.x / ngroups;
    const int64_t nblock = ngroup * 4 + wv;
    const int64_t n0 = nblock * kSamplePad;
    if (n0 >= Npad) return;
    const int64_t m_begin = wchunk * rows_per_wave;
    const int64_t m_end = (m_begin + rows_per_wave < Mpad) ? m_begin + rows_per_wave : Mpad;
    const int64_t groups = (m_end - m_begin) >> 4;   // even: Mpad and rows_per_wave are multiples of 32

    f32x16 acc[8][LT];
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int lt = 0; lt < LT; ++lt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[t][lt][e] = 0.f;

    // (ldg = row pitch in bytes: N padded for int8 rows, a quarter of it for packed rows)
    const uint32_t gvo = PACKED ? (uint32_t)(h * ldg + 4 * (c >> 1)) : (uint32_t)(h * ldg + 8 * c);
    const unsigned hsh = 16u * (unsigned)(c & 1);
    const uint32_t tvo = (uint32_t)(lane * 32);
    constexpr uint32_t TGR = LT * 2048;                       // bytes of Tb per 16-row group
    const uint8_t* gp = G + m_begin * ldg + (PACKED ? (n0 >> 2) : n0);
    const char* tp = reinterpret_cast<const char*>(Tb) + (m_begin >> 4) * TGR;
    GttBuf<LT> A, B;
    gtt_load<LT, PACKED>(A, make_rsrc(gp), gvo, 0u, (uint32_t)ldg, make_rsrc(tp), tvo, 0u);
    for (int64_t g = 0; g < groups; g += 2) {
        // descriptors are re-based every pair of groups, so the 32-bit offsets stay < 48 * ldg
        const __amdgpu_buffer_rsrc_t rg = make_rsrc(gp + g * 16 * ldg);
        const __amdgpu_buffer_rsrc_t rt = make_rsrc(tp + g * TGR);
        const uint32_t nx = (g + 2 < groups) ? 2u : 0u;       // last pair prefetches its own first group (unused)
        gtt_load<LT, PACKED>(B, rg, gvo, 16u * (uint32_t)ldg, (uint32_t)ldg, rt, tvo, TGR);
        __builtin_amdgcn_sched_barrier(0);
        gtt_compute<LT, PACKED>(A, acc, hsh);
        __builtin_amdgcn_sched_barrier(0);
        gtt_load<LT, PACKED>(A, rg, gvo, 16u * nx * (uint32_t)ldg, (uint32_t)ldg, rt, tvo, TGR * nx);
        __builtin_amdgcn_sched_barrier(0);
        gtt_compute<LT, PACKED>(B, acc, hsh);
        __builtin_amdgcn_sched_barrier(0);
    }
    // D[j][col]: j = (reg&3) + 8*(reg>>2) + 4*h (+32 lt), col = c -> sample n0 + 8c + t.
    // regs e..e+3 are 4 consecutive j: one 16-byte store per (tile, quad).  (The 2^9 of the fp8 trick is applied
    // by k_reduce_y.)
    float* yp = Ypart + (wchunk * Npad) * L;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int64_t n = n0 + 8 * c + t;
#pragma unroll
        for (int lt = 0; lt < LT; ++lt)
#pragma unroll
            for (int e = 0; e < 16; e += 4) {
                const int j = acc_row(32 * lt, e, h);
                float4 o;
                o.x = acc[t][lt][e]; o.y = acc[t][lt][e + 1]; o.z = acc[t][lt][e + 2]; o.w = acc[t][lt][e + 3];
                *reinterpret_cast<float4*>(yp + n * L + j) = o;
            }
    }
}

void launch_gtt_f32(hipStream_t st, const void* G, int packed, int64_t ldr, int64_t Mpad, int64_t Npad, const float* Tb, int L,
                    float* Ypart, const GttPlan& plan) {
    const int64_t ngroups = (plan.nblocks_n + 3) / 4;
    const dim3 grid((unsigned)plan.grid), blk(256);
#define GPCA_GTTF(LTV, PK) hipLaunchKernelGGL((k_gtt_f32<LTV, PK>), grid, blk, 0, st, (const uint8_t*)G, ldr, Mpad, Npad, Tb, Ypart, ngroups, plan.rows_per_wave)
    if (L == 32) { if (packed) GPCA_GTTF(1, true); else GPCA_GTTF(1, false); }
    else { if (packed) GPCA_GTTF(2, true); else GPCA_GTTF(2, false); }
#undef GPCA_GTTF
}

}  // namespace gpca
