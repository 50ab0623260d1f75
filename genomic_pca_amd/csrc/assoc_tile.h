// The tile and stage pipeline of the two mainloop association kernels, k_assoc (assoc.hip) and k_assoc_score (assoc_score.hip).
//
// A workgroup of kAscThreads = 256 threads owns kAscRows = 128 kept rows x all columns of the panel B, 4 waves of 32 rows x 32 NB
// columns, and walks the samples in stages of kAscStage = 64.  A stage in LDS is the staged bytes [row][sample] (an operand 0, 1, 2 or
// the missing code; an excluded sample and a sample past N are 0) and the panel of B^T [column][sample].  Staging map: thread t carries
// 32 samples (half t & 1 of the stage) of row t / 2; what it writes for them is the caller's stager, called once per staged 32 samples
// with (F, inb, inc, dst).  Two LDS buffers: the waves multiply stage s from one while stage s + 1 (fetched during stage s - 1) is
// written to the other and stage s + 2 is requested, one barrier per stage.
// A lane reads 8 consecutive samples of its row (ds_read_b64) and of its column (2 x ds_read_b128) and turns the bytes into the f32
// operands x and [missing] in registers, so every product of the v_mfma_f32_32x32x2_f32 is exact.  The 16 samples of a group of 8
// multiplies are taken as (i, 8 + i), i = 0 .. 7: the order is a function of the sample index alone.  Per 16-sample group and column
// block: d += x B, then (WITH_Q, column block 0 only) q += x^2 B, then e += [missing] B, the last only in groups where a wave ballot
// finds a missing call.  Every kAscFlush = 256 samples, counted from sample 0, and after the last stage the f32 accumulators are added
// to the f64 running sums, which belong to the caller: its epilogue reads them when the pipeline returns (the last barrier passed).
// A translation unit that includes this header keeps floating-point contraction off (#pragma clang fp contract(off)).
#pragma once
#include "assoc_stage.h"

namespace gpca {

// NS: the words per row of the caller's own per-row sums
template <int NB, int NS>
struct AscSmem {
    uint8_t g[2][kAscRows * kAscGPitch];
    float b[2][NB * 32 * kAscBPitch];
    unsigned sums[kAscRows * NS];
};

// the row of the tile that accumulator element e (of any column block) of wave wv holds in lane half h = lane >> 5; its column is
// 32 j + (lane & 31) in column block j
__device__ __forceinline__ int asc_acc_row(int wv, int h, int e) { return acc_row(32 * wv, e, h); }

// sorow: the original row that this thread stages (-1: none, zeros are staged); Bt [32 NB][npad]; rd, re and (WITH_Q) rq [16]: the
// caller's running sums, zeroed here (rq is not touched without WITH_Q); wv, lane: the thread's wave (wave-uniform) and lane
template <bool PACKED, int NB, bool WITH_Q, int NS, class Stager>
__device__ __forceinline__ void asc_pipeline(AscSmem<NB, NS>& sm, const uint8_t* G, int64_t ldr, int64_t sorow, int64_t N,
                                             int64_t npad, const float* Bt, const unsigned* incw, Stager&& put,
                                             double (&rd)[NB][16], double (&re)[NB][16], double* rq, int wv, int lane) {
    const int c = lane & 31, h = lane >> 5;
    const int srow = threadIdx.x >> 1, sh = threadIdx.x & 1;
    auto inb_of = [&](int64_t s) { return asc_inb(N, s * kAscStage + 32 * sh); };
    auto inc_of = [&](int64_t s) { return incw[s * (kAscStage / 32) + sh]; };

    f32x16 ad[NB], ae[NB], aq;
    if constexpr (WITH_Q) {
#pragma unroll
        for (int e = 0; e < 16; ++e) { aq[e] = 0.0f; rq[e] = 0.0; }
    }
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
    put(F, inb_of(0), inc_of(0), sm.g[0] + sg_off);
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
            if constexpr (WITH_Q) {
#pragma unroll
                for (int i = 0; i < 8; ++i) g2[i] = gf[i] * gf[i];
            }
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const f32x4 b0 = *reinterpret_cast<const f32x4*>(lb + 32 * j * kAscBPitch + 16 * q);
                const f32x4 b1 = *reinterpret_cast<const f32x4*>(lb + 32 * j * kAscBPitch + 16 * q + 4);
#pragma unroll
                for (int i = 0; i < 8; ++i) ad[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(gf[i], i < 4 ? b0[i] : b1[i - 4], ad[j], 0, 0, 0);
                if constexpr (WITH_Q) {
                    if (j == 0) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) aq = __builtin_amdgcn_mfma_f32_32x32x2f32(g2[i], i < 4 ? b0[i] : b1[i - 4], aq, 0, 0, 0);
                    }
                }
                if (anym) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) ae[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(mf[i], i < 4 ? b0[i] : b1[i - 4], ae[j], 0, 0, 0);
                }
            }
        }
        if ((s + 1) % (kAscFlush / kAscStage) == 0 || s + 1 == nst) {
            if constexpr (WITH_Q) {
#pragma unroll
                for (int e = 0; e < 16; ++e) { rq[e] += (double)aq[e]; aq[e] = 0.0f; }
            }
#pragma unroll
            for (int j = 0; j < NB; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    rd[j][e] += (double)ad[j][e]; ad[j][e] = 0.0f;
                    re[j][e] += (double)ae[j][e]; ae[j][e] = 0.0f;
                }
        }
        if (s + 1 < nst) {
            put(F, inb_of(s + 1), inc_of(s + 1), sm.g[(s + 1) & 1] + sg_off);
            asc_put_b<NB>(P, sm.b[(s + 1) & 1]);
        }
        if (s + 2 < nst) {
            asc_fetch<PACKED>(F, G, ldr, sorow, (s + 2) * kAscStage + 32 * sh);
            asc_fetch_b<NB>(P, Bt, npad, (s + 2) * kAscStage);
        }
        __syncthreads();
    }
}

}  // namespace gpca
