// The staging helpers of the association kernels (assoc.hip, assoc_score.hip, assoc_spa.hip, assoc_firth.hip): the fetch of 32 samples of a
// row from either storage, the check / mask / count of those samples on their way into a stage's LDS buffer, the staging of one item's
// covariate-adjusted genotype for the two corrections, and the fetch and store of a stage's panel of B^T.
// (assoc_tile.h holds the stage pipeline that the two mainloop kernels build from them.)
#pragma once
#include "syrk_tile.h"

namespace gpca {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr unsigned kAscMissing = kMissingByte;

// the 32 samples a thread stages: 8 dwords of call bytes (int8 storage: as stored; 2-bit: decoded, 3 -> the missing code)
struct AscFetch { unsigned w[8]; };

template <bool PACKED>
__device__ __forceinline__ void asc_fetch(AscFetch& F, const uint8_t* __restrict__ G, int64_t ldr, int64_t orow, int64_t ns) {
    if (orow < 0) {
#pragma unroll
        for (int d = 0; d < 8; ++d) F.w[d] = 0u;
        return;
    }
    if (PACKED) {
        // (ns is a multiple of 32 and ld2 of 256: the 8 bytes are aligned and inside the row's pitch, see asc_* in plan_math.h)
        const uint2 v = *reinterpret_cast<const uint2*>(G + orow * ldr + (ns >> 2));
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            const unsigned b = ((d < 4 ? v.x : v.y) >> (8 * (d & 3))) & 0xffu;
            F.w[d] = unpack4(b);
        }
    } else {
        const uint4 a = *reinterpret_cast<const uint4*>(G + orow * ldr + ns);
        const uint4 b = *reinterpret_cast<const uint4*>(G + orow * ldr + ns + 16);
        F.w[0] = a.x; F.w[1] = a.y; F.w[2] = a.z; F.w[3] = a.w; F.w[4] = b.x; F.w[5] = b.y; F.w[6] = b.z; F.w[7] = b.w;
    }
}

// the "samples left of N" mask of the 32 samples that start at n0: bit s = sample n0 + s lies below N
__device__ __forceinline__ unsigned asc_inb(int64_t N, int64_t n0) {
    const int64_t left = N - n0;
    return left >= 32 ? 0xffffffffu : (left <= 0 ? 0u : (1u << (int)left) - 1u);
}

// checks, masks and counts the thread's 32 samples: o = the bytes a stage holds (an excluded sample and a sample past N are 0).
// inb: bit s = sample s lies below N; inc: bit s = sample s is included (zero past N).
__device__ __forceinline__ void asc_mask_count(const AscFetch& F, unsigned inb, unsigned inc, unsigned (&o)[8], unsigned& nobs, unsigned& s1,
                                               unsigned& s2, unsigned& bd) {
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        const unsigned vb = kept_bytes(inb, d) * 0xffu;
        const unsigned ib = kept_bytes(inc, d) * 0xffu;
        const unsigned a = F.w[d] & vb;
        // valid bytes: 0, 1, 2 and the missing code
        const unsigned m = (a >> 7) & 0x01010101u, g = a & ~(m * 0xffu);
        if ((a & (m * 0xffu)) != m * kAscMissing || (g & 0xfcfcfcfcu) != 0u || (g & (g >> 1) & 0x01010101u) != 0u) bd = 1u;
        const unsigned ai = a & ib, mi = (ai >> 7) & 0x01010101u, gi = ai & ~(mi * 0xffu);
        const unsigned c1 = __builtin_popcount(gi & 0x01010101u), c2 = __builtin_popcount(gi & 0x02020202u);
        nobs += __builtin_popcount((inc >> (4 * d)) & 0xfu) - __builtin_popcount(mi);
        s1 += c1 + 2u * c2;
        s2 += c1 + 4u * c2;
        o[d] = ai;
    }
}
// ... and writes them to the stage's buffer
__device__ __forceinline__ void asc_put(const AscFetch& F, unsigned inb, unsigned inc, uint8_t* dst, unsigned& nobs, unsigned& s1,
                                        unsigned& s2, unsigned& bd) {
    unsigned o[8];
    asc_mask_count(F, inb, inc, o, nobs, s1, s2, bd);
#pragma unroll
    for (int d = 0; d < 4; ++d) *reinterpret_cast<uint2*>(dst + 8 * d) = make_uint2(o[2 * d], o[2 * d + 1]);
}

// masks the thread's 32 samples, recodes them to the operand (flip: 2 - g where observed) and writes them to the stage's buffer
__device__ __forceinline__ void asr_put(const AscFetch& F, unsigned inb, unsigned inc, bool flip, uint8_t* dst) {
    unsigned o[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        const unsigned vb = kept_bytes(inb, d) * 0xffu;
        const unsigned ib = kept_bytes(inc, d) * 0xffu;
        const unsigned a = F.w[d] & vb & ib;
        const unsigned m = (a >> 7) & 0x01010101u, g = a & ~(m * 0xffu);
        // (a valid byte of g is 0, 1 or 2: 2 - g borrows nothing from its neighbour; an invalid one fails the call in the count kernel)
        const unsigned x = flip ? ((0x02020202u - g) & vb & ib & ~(m * 0xffu)) : g;
        o[d] = x | (m * kAscMissing);
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) *reinterpret_cast<uint2*>(dst + 8 * d) = make_uint2(o[2 * d], o[2 * d + 1]);
}

// The covariate-adjusted genotype g~ of one (row, trait) item, staged by a workgroup of kAspThreads threads (k_assoc_spa, k_assoc_firth;
// include/gpca.h section a14, "Setting").  The row is read once, in chunks of kAspChunk samples: a thread fetches 32 samples
// (asc_fetch) and masks and flips them as the score kernel does (asr_put) into sx [kAspChunk]; then thread t owns the samples
// t + kAspThreads k: x~ = the operand, xbar on a missing call, 0 outside S; g~ = x~ - sum_j sa[j] Z_nj (j ascending, f64, no fused
// multiply-add), written to gw [npad]; each(n, g~) sees every sample the thread owns, in ascending order.  sa [P] is written by the
// caller before the call (the first barrier here orders it); g~ is visible to the workgroup after the caller's next barrier.
template <bool PACKED, class Each>
__device__ __forceinline__ void asp_stage_gt(const uint8_t* __restrict__ G, int64_t ldr, int64_t orow, int64_t N, int64_t npad,
                                             const unsigned* __restrict__ incw, bool flip, double xbar, const double* sa, int P,
                                             const double* __restrict__ Zt, uint8_t* sx, double* gw, Each&& each) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    for (int64_t c0 = 0; c0 < npad; c0 += kAspChunk) {
        const int64_t n0 = c0 + 32 * tid;
        // (n0 is a multiple of 32 below npad: the read stays inside the row's pitch and the include word exists, as in k_assoc)
        if (n0 < npad) {
            AscFetch F;
            asc_fetch<PACKED>(F, G, ldr, orow, n0);
            asr_put(F, asc_inb(N, n0), incw[n0 >> 5], flip, sx + 32 * tid);
        }
        __syncthreads();                                                    // (also orders sa before its first use)
#pragma nounroll
        for (int k = 0; k < 32; ++k) {
            const int64_t n = c0 + tid + kAspThreads * k;
            if (n >= npad) break;
            const unsigned b = sx[tid + kAspThreads * k];
            const double xt = b == kAscMissing ? xbar : (double)b;
            double acc = 0.0;
            for (int j = 0; j < P; ++j) acc = acc + sa[j] * Zt[(int64_t)j * npad + n];
            const double gg = xt - acc;
            gw[n] = gg;
            each(n, gg);
        }
        __syncthreads();
    }
}

// Bt [32 NB][npad]: the panel of a stage is 32 NB columns x 16 float4
template <int NB>
__device__ __forceinline__ void asc_fetch_b(f32x4 (&P)[2 * NB], const float* __restrict__ Bt, int64_t npad, int64_t n0) {
#pragma unroll
    for (int i = 0; i < 2 * NB; ++i) {
        const int idx = threadIdx.x + kAscThreads * i;
        P[i] = *reinterpret_cast<const f32x4*>(Bt + (int64_t)(idx >> 4) * npad + n0 + 4 * (idx & 15));
    }
}
template <int NB>
__device__ __forceinline__ void asc_put_b(const f32x4 (&P)[2 * NB], float* dst) {
#pragma unroll
    for (int i = 0; i < 2 * NB; ++i) {
        const int idx = threadIdx.x + kAscThreads * i;
        *reinterpret_cast<f32x4*>(dst + (idx >> 4) * kAscBPitch + 4 * (idx & 15)) = P[i];
    }
}

}  // namespace gpca
