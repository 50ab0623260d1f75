// Per-sample genotype counts (gpca_sample_counts; gpca_sample_counts.cpp; include/gpca.h section a18): for every sample, over the kept
// rows of a band, the exact counts of observed, heterozygous and homozygous-A1 calls and, with weights q, the sum of q over the rows on
// which the sample is observed.
//
// A column reduction: the sample axis is contiguous in both residencies, so a thread that owns kScLane = 16 consecutive samples reads
// one uint4 of an int8 row or one dword of a 2-bit row, a wave reads 1 KiB (256 B) of consecutive bytes per row, and nothing is
// transposed, staged in LDS or multiplied.  k_sample_counts: workgroup b (one wave) owns the chunk b % chunks of kScChunk samples and
// the row split b / chunks (sc_plan in plan_math.h); it walks its split's kept rows through krows, kScUnroll rows' loads in flight.
// Per row and dword of four calls: m = the missing bytes' bit 7, het = bit 0 of the bytes that are not missing, hom2 = bit 1; each is
// added to a dword of four byte counters (SWAR), and the byte counters are added to u32 registers once per kScFlushRows < 256 rows,
// before a byte can wrap.  With weights, sum over observed = (sum of all q of the band, formed on the host) - (sum of q over the
// sample's missing calls): the per-sample u64 adds run only on rows where a wave ballot finds a missing call among the wave's samples.
// No float touches a sum.  A sample at or beyond N is masked to 0 before it is checked or counted.
// The row splits meet in slabs: a thread writes its 16 x (missing, het, hom2) and its 16 u64 once, with plain 16-byte stores, to the slab
// of its split; k_sc_sum adds the slabs of a sample, splits ascending, and writes n_obs = rows - missing, n_het, n_hom2 and
// qsum = qtot - (the missing calls' q).  Integer sums: the split count changes no bit.  (Slabs, not atomics: see DESIGN section 7.)
// Registers: the figures hipcc reports are in DESIGN section 7.
#include "syrk_tile.h"

namespace gpca {

// the 16 calls a thread fetches of one row
template <bool PACKED> struct ScFetch;
template <> struct ScFetch<false> { uint4 v; };
template <> struct ScFetch<true> { unsigned v; };

// (base = the row-0 address of the thread's fetch, sc_row_offset: 16-byte (4-byte) aligned and inside the row's pitch)
__device__ __forceinline__ void sc_fetch(ScFetch<false>& F, const uint8_t* __restrict__ base, int64_t ldr, int64_t orow) {
    F.v = *reinterpret_cast<const uint4*>(base + orow * ldr);
}
__device__ __forceinline__ void sc_fetch(ScFetch<true>& F, const uint8_t* __restrict__ base, int64_t ldr, int64_t orow) {
    F.v = *reinterpret_cast<const unsigned*>(base + orow * ldr);
}
__device__ __forceinline__ unsigned sc_dword(const ScFetch<false>& F, int d) { return d == 0 ? F.v.x : d == 1 ? F.v.y : d == 2 ? F.v.z : F.v.w; }
__device__ __forceinline__ unsigned sc_dword(const ScFetch<true>& F, int d) { return unpack4((F.v >> (8 * d)) & 0xffu); }

// one row of the thread's 16 samples: vb = the byte masks of the samples below N; sw [3][4] = the byte counters (missing, het, hom2);
// qm = the u64 sums of q over the missing calls; returns nonzero iff a sample below N holds a value outside {0, 1, 2, missing}
template <bool PACKED, bool HASQ>
__device__ __forceinline__ unsigned sc_row(const ScFetch<PACKED>& F, const unsigned (&vb)[4], unsigned (&sw)[3][4], unsigned qv,
                                           unsigned long long (&qm)[kScLane]) {
    unsigned mm[4], anym = 0u, bd = 0u;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const unsigned a = sc_dword(F, d) & vb[d];
        const unsigned m = (a >> 7) & 0x01010101u;
        // valid bytes: 0, 1, 2 and the missing code 0x81 (2-bit storage decodes to nothing else): bits 2 .. 6 clear, not (bit 1 and
        // bit 0), and bit 7 only with bit 0 set and bit 1 clear
        if (!PACKED) bd |= (a & 0x7c7c7c7cu) | ((((a >> 1) & a) | (m & ((a >> 1) | ~a))) & 0x01010101u);
        sw[0][d] += m;
        sw[1][d] += a & ~m & 0x01010101u;                                          // (the missing code has bit 0 set)
        sw[2][d] += (a >> 1) & 0x01010101u;
        mm[d] = m;
        anym |= m;
    }
    if (HASQ) {
        if (__builtin_amdgcn_ballot_w64(anym != 0u) != 0ull) {                      // wave-uniform
#pragma unroll
            for (int d = 0; d < 4; ++d)
#pragma unroll
                for (int j = 0; j < 4; ++j) qm[4 * d + j] += ((mm[d] >> (8 * j)) & 1u) ? (unsigned long long)qv : 0ull;
        }
    }
    return bd;
}

// part [splits][npad][3] u32 and qpart [splits][npad] u64 of kept rows [row0, row1) in splits of `per` rows; q [row1 - row0] or unused;
// *bad = min original row with a value outside {0, 1, 2, missing} on a sample below N
template <bool PACKED, bool HASQ>
__global__ __launch_bounds__(kScThreads) void k_sample_counts(const void* __restrict__ Gv, int64_t ldr, const int64_t* __restrict__ krows,
                                                              int64_t N, int64_t npad, int64_t chunks, const unsigned* __restrict__ q,
                                                              int64_t row0, int64_t row1, int64_t per, unsigned* __restrict__ part,
                                                              unsigned long long* __restrict__ qpart, unsigned long long* __restrict__ bad) {
    const int64_t chunk = (int64_t)blockIdx.x % chunks, split = (int64_t)blockIdx.x / chunks;
    const int64_t n0 = sc_thread_sample(chunk, threadIdx.x);
    if (n0 >= npad) return;
    const int64_t ka = row0 + split * per, kb = ka + per < row1 ? ka + per : row1;
    const int64_t left = N - n0;
    const unsigned inb = left >= kScLane ? 0xffffu : (1u << (int)left) - 1u;       // (n0 < npad: left >= 1)
    unsigned vb[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) vb[d] = kept_bytes(inb, d) * 0xffu;
    const uint8_t* base = (const uint8_t*)Gv + sc_row_offset(PACKED, n0);

    unsigned acc[3][kScLane];
    unsigned long long qm[kScLane];
#pragma unroll
    for (int s = 0; s < kScLane; ++s) { acc[0][s] = 0u; acc[1][s] = 0u; acc[2][s] = 0u; qm[s] = 0ull; }

    for (int64_t k = ka; k < kb;) {
        const int64_t kend = k + kScFlushRows < kb ? k + kScFlushRows : kb;
        unsigned sw[3][4];
#pragma unroll
        for (int d = 0; d < 4; ++d) { sw[0][d] = 0u; sw[1][d] = 0u; sw[2][d] = 0u; }
        for (; k + kScUnroll <= kend; k += kScUnroll) {
            ScFetch<PACKED> F[kScUnroll];
            int64_t orow[kScUnroll];
#pragma unroll
            for (int u = 0; u < kScUnroll; ++u) { orow[u] = krows[k + u]; sc_fetch(F[u], base, ldr, orow[u]); }
#pragma unroll
            for (int u = 0; u < kScUnroll; ++u)
                if (sc_row<PACKED, HASQ>(F[u], vb, sw, HASQ ? q[k + u - row0] : 0u, qm)) atomicMin(bad, (unsigned long long)orow[u]);
        }
        for (; k < kend; ++k) {
            ScFetch<PACKED> F;
            const int64_t orow = krows[k];
            sc_fetch(F, base, ldr, orow);
            if (sc_row<PACKED, HASQ>(F, vb, sw, HASQ ? q[k - row0] : 0u, qm)) atomicMin(bad, (unsigned long long)orow);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int d = 0; d < 4; ++d)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[c][4 * d + j] += (sw[c][d] >> (8 * j)) & 0xffu;
    }

    // 48 u32 = 12 uint4 at sc_part_index(split, npad, n0, 0): a multiple of 48 elements, 16-byte aligned
    uint4* po = reinterpret_cast<uint4*>(part + sc_part_index(split, npad, n0, 0));
    unsigned o[3 * kScLane];
#pragma unroll
    for (int s = 0; s < kScLane; ++s) { o[3 * s] = acc[0][s]; o[3 * s + 1] = acc[1][s]; o[3 * s + 2] = acc[2][s]; }
#pragma unroll
    for (int i = 0; i < 3 * kScLane / 4; ++i) po[i] = make_uint4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
    if (HASQ) {
        ulonglong2* qo = reinterpret_cast<ulonglong2*>(qpart + sc_qpart_index(split, npad, n0));
#pragma unroll
        for (int i = 0; i < kScLane / 2; ++i) qo[i] = make_ulonglong2(qm[2 * i], qm[2 * i + 1]);
    }
}

// counts [N][3] = rows - sum missing, sum het, sum hom2 and qsum [N] = qtot - sum qpart over the splits, ascending; a thread per sample
__global__ __launch_bounds__(kScSumThreads) void k_sc_sum(const unsigned* __restrict__ part, const unsigned long long* __restrict__ qpart,
                                                          int64_t N, int64_t npad, int64_t splits, unsigned rows, unsigned long long qtot,
                                                          unsigned* __restrict__ counts, unsigned long long* __restrict__ qsum) {
    const int64_t n = (int64_t)blockIdx.x * kScSumThreads + threadIdx.x;
    if (n >= N) return;
    unsigned mis = 0u, het = 0u, hom = 0u;
    unsigned long long qs = 0ull;
    for (int64_t s = 0; s < splits; ++s) {
        const unsigned* p = part + sc_part_index(s, npad, n, 0);
        mis += p[0]; het += p[1]; hom += p[2];
        if (qpart) qs += qpart[sc_qpart_index(s, npad, n)];
    }
    counts[3 * n] = rows - mis; counts[3 * n + 1] = het; counts[3 * n + 2] = hom;
    if (qpart) qsum[n] = qtot - qs;
}

int launch_sample_counts(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t N, const unsigned* q,
                         int64_t row0, int64_t row1, const ScPlan& plan, unsigned* part, unsigned long long* qpart,
                         unsigned long long* bad) {
    const int64_t rows = row1 - row0;
    if (rows <= 0) return 0;
    if (N < 1 || rows >= ((int64_t)1 << 31) || plan.chunks != sc_chunks(N) || plan.per < 1 || plan.splits < 1 ||
        (plan.splits - 1) * plan.per >= rows || plan.splits * plan.per < rows || sc_grid(plan) >= ((int64_t)1 << 31) || (q && !qpart))
        return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)sc_grid(plan)), blk(kScThreads);
    const int64_t npad = sc_npad(N);
#define GPCA_SC(PK, HQ) hipLaunchKernelGGL((k_sample_counts<PK, HQ>), grid, blk, 0, st, G, ldr, krows, N, npad, plan.chunks, q, row0, row1, plan.per, part, qpart, bad)
    if (q) { if (packed) GPCA_SC(true, true); else GPCA_SC(false, true); }
    else { if (packed) GPCA_SC(true, false); else GPCA_SC(false, false); }
#undef GPCA_SC
    return 0;
}

void launch_sc_sum(hipStream_t st, const unsigned* part, const unsigned long long* qpart, int64_t N, int64_t splits, int64_t rows,
                   unsigned long long qtot, unsigned* counts, unsigned long long* qsum) {
    hipLaunchKernelGGL(k_sc_sum, dim3((unsigned)((N + kScSumThreads - 1) / kScSumThreads)), dim3(kScSumThreads), 0, st, part, qpart, N,
                       sc_npad(N), splits, (unsigned)rows, qtot, counts, qsum);
}

}  // namespace gpca
