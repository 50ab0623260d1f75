// Per-group genotype counts (gpca_group_counts; gpca_group_counts.cpp; include/gpca.h section a17): for every kept row of a band and
// every one of P <= 64 sample groups, the exact counts of observed, heterozygous and homozygous-A1 calls.
//
// The counts are three products of 0/1 bytes over the sample axis, on v_mfma_i32_32x32x32_i8:
//     het[i][p] = sum_n [g_in == 1] O_pn,   hom[i][p] = sum_n [g_in == 2] O_pn,   mis[i][p] = sum_n [g_in missing] O_pn
// with O [gc_ppad(P)][gc_npad(N)] the one-hot matrix of the labels (k_gc_onehot: O_pn = 1 iff n < N and group[n] == p; a sample with
// label -1, a pad sample and a pad column are all zero, so whatever a row's pad bytes hold adds nothing), and
//     n_obs[i][p] = size[p] - mis[i][p],   size[p] = the samples of group p (counted on the host).
// The sample axis is the K axis of the instruction and it is contiguous in both residencies and in O, so a lane's 16 operand bytes are
// 16 bytes of the staged row (or of the staged one-hot column) as they are: no transpose.
// k_group_counts: a workgroup owns kGcRows kept rows (wave w: rows 32 w .. 32 w + 31) and all column blocks; it stages kGcStage samples
// of its rows (asc_fetch: the scans' fetch from either storage; gc_put checks the bytes below N and zeroes the ones past N) and of
// O's columns through two LDS buffers, one barrier per stage, the global loads of stage s + 2 issued while stage s multiplies.  Per
// block of kGcBlock samples a wave issues two MFMAs per column block (het, hom) and, where a wave ballot over its 32 rows finds a
// missing call in the block, a third (mis).  NB = 2 column blocks share the row operands: the genotypes are read once for P > 32.
// i32 accumulators, exact for N < 2^31 (the call refuses N >= 2^30); no split of the sample axis and no atomics: a count is written
// once, by the wave that owns its row, and depends on the row, the labels and N alone.
// Registers: 3 x NB x 16 i32 accumulators per lane; the figures hipcc reports are in DESIGN section 7.
#include "assoc_stage.h"

namespace gpca {

// O [ppad][npad] from the labels: a thread writes four samples of one column
__global__ __launch_bounds__(256) void k_gc_onehot(const int32_t* __restrict__ group, int64_t N, int64_t npad, int ppad,
                                                   uint8_t* __restrict__ O) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;                      // (the dword q of column blockIdx.y)
    const int p = blockIdx.y;
    if (q >= npad / 4 || p >= ppad) return;
    unsigned v = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t n = 4 * q + k;
        if (n < N && group[n] == p) v |= 1u << (8 * k);
    }
    *reinterpret_cast<unsigned*>(O + (int64_t)p * npad + 4 * q) = v;
}
void launch_gc_onehot(hipStream_t st, const int32_t* group, int64_t N, int P, uint8_t* O) {
    const int64_t npad = gc_npad(N);
    hipLaunchKernelGGL(k_gc_onehot, dim3((unsigned)((npad / 4 + 255) / 256), (unsigned)gc_ppad(P)), dim3(256), 0, st, group, N, npad, gc_ppad(P), O);
}

template <int NB>
struct GcSmem {
    uint8_t g[2][kGcRows * kGcPitch];
    uint8_t o[2][32 * NB * kGcPitch];
};

// checks the thread's 32 samples (those below N: inb) and writes them to the stage's buffer, zero past N
__device__ __forceinline__ void gc_put(const AscFetch& F, unsigned inb, uint8_t* dst, unsigned& bd) {
    unsigned o[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        const unsigned vb = kept_bytes(inb, d) * 0xffu;
        const unsigned a = F.w[d] & vb;
        // valid bytes: 0, 1, 2 and the missing code
        const unsigned m = (a >> 7) & 0x01010101u, g = a & ~(m * 0xffu);
        if ((a & (m * 0xffu)) != m * kMissingByte || (g & 0xfcfcfcfcu) != 0u || (g & (g >> 1) & 0x01010101u) != 0u) bd = 1u;
        o[d] = a;
    }
#pragma unroll
    for (int d = 0; d < 2; ++d) *reinterpret_cast<uint4*>(dst + 16 * d) = make_uint4(o[4 * d], o[4 * d + 1], o[4 * d + 2], o[4 * d + 3]);
}

// counts [row1 - row0][P][3] u32 of kept rows [row0, row1); size [P] = the samples of each group; *bad = min original row with a value
// outside {0, 1, 2, missing} on a sample below N
template <bool PACKED, int NB>
__global__ __launch_bounds__(kGcThreads) void k_group_counts(const void* __restrict__ Gv, int64_t ldr, const int64_t* __restrict__ krows,
                                                             int64_t N, int64_t npad, const uint8_t* __restrict__ O,
                                                             const unsigned* __restrict__ size, int P, int64_t row0, int64_t row1,
                                                             unsigned* __restrict__ counts, unsigned long long* __restrict__ bad) {
    __shared__ __attribute__((aligned(16))) GcSmem<NB> sm;
    const uint8_t* G = (const uint8_t*)Gv;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int64_t k0 = row0 + (int64_t)blockIdx.x * kGcRows;

    // the staging map: this thread stages half sh of row srow, and (below 4 x 32 NB threads) quarter oq of one-hot column oc
    const int srow = threadIdx.x >> 1, sh = threadIdx.x & 1;
    const int64_t sorow = k0 + srow < row1 ? krows[k0 + srow] : -1;
    const int oc = threadIdx.x >> 2, oq = threadIdx.x & 3;
    const bool olive = oc < 32 * NB;
    const int sg_off = srow * kGcPitch + 32 * sh, so_off = oc * kGcPitch + 16 * oq;
    unsigned bd = 0u;

    i32x16 het[NB], hom[NB], mis[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) { het[j][e] = 0; hom[j][e] = 0; mis[j][e] = 0; }

    const int64_t nst = gc_stages(N);
    const int a_off = (32 * wv + c) * kGcPitch + 16 * h, b_off = c * kGcPitch + 16 * h;

    AscFetch F;
    uint4 OF = make_uint4(0u, 0u, 0u, 0u);
    // (a fetch at sample ns < npad, a multiple of 32, stays inside the row's pitch; a column of O holds npad bytes: gc_* in plan_math.h)
    asc_fetch<PACKED>(F, G, ldr, sorow, 32 * sh);
    if (olive) OF = *reinterpret_cast<const uint4*>(O + gc_onehot_offset(npad, threadIdx.x, 0));
    gc_put(F, asc_inb(N, 32 * sh), sm.g[0] + sg_off, bd);
    if (olive) *reinterpret_cast<uint4*>(sm.o[0] + so_off) = OF;
    if (nst > 1) {
        asc_fetch<PACKED>(F, G, ldr, sorow, kGcStage + 32 * sh);
        if (olive) OF = *reinterpret_cast<const uint4*>(O + gc_onehot_offset(npad, threadIdx.x, 1));
    }
    __syncthreads();
    for (int64_t s = 0; s < nst; ++s) {
        const uint8_t* la = sm.g[s & 1] + a_off;
        const uint8_t* lb = sm.o[s & 1] + b_off;
#pragma unroll
        for (int q = 0; q < kGcStage / kGcBlock; ++q) {
            const i32x4 va = *reinterpret_cast<const i32x4*>(la + kGcBlock * q);
            i32x4 H1, H2, M;
            unsigned anym = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned a = (unsigned)va[k];
                const unsigned m = (a >> 7) & 0x01010101u;
                H1[k] = (int)(a & ~m & 0x01010101u);                                // (the missing code has bit 0 set)
                H2[k] = (int)((a >> 1) & 0x01010101u);
                M[k] = (int)m;
                anym |= m;
            }
            const bool miss = __builtin_amdgcn_ballot_w64(anym != 0u) != 0ull;     // wave-uniform
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const i32x4 vb = *reinterpret_cast<const i32x4*>(lb + 32 * j * kGcPitch + kGcBlock * q);
                het[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(H1, vb, het[j], 0, 0, 0);
                hom[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(H2, vb, hom[j], 0, 0, 0);
                if (miss) mis[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(M, vb, mis[j], 0, 0, 0);
            }
        }
        if (s + 1 < nst) {                                                          // (its last readers finished before the previous barrier)
            gc_put(F, asc_inb(N, (s + 1) * kGcStage + 32 * sh), sm.g[(s + 1) & 1] + sg_off, bd);
            if (olive) *reinterpret_cast<uint4*>(sm.o[(s + 1) & 1] + so_off) = OF;
        }
        if (s + 2 < nst) {
            asc_fetch<PACKED>(F, G, ldr, sorow, (s + 2) * kGcStage + 32 * sh);
            if (olive) OF = *reinterpret_cast<const uint4*>(O + gc_onehot_offset(npad, threadIdx.x, s + 2));
        }
        __syncthreads();
    }
    if (bd && sorow >= 0) atomicMin(bad, (unsigned long long)sorow);

#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int p = 32 * j + c;
        if (p >= P) continue;
        const unsigned sz = size[p];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int64_t kr = k0 + acc_row(32 * wv, e, h);
            if (kr >= row1) continue;
            unsigned* o = counts + gc_counts_index(kr - row0, P, p, 0);
            o[0] = sz - (unsigned)mis[j][e]; o[1] = (unsigned)het[j][e]; o[2] = (unsigned)hom[j][e];
        }
    }
}

int launch_group_counts(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t N, const uint8_t* O,
                        const unsigned* size, int P, int64_t row0, int64_t row1, unsigned* counts, unsigned long long* bad) {
    if (row1 <= row0) return 0;
    const int64_t nb = gc_row_blocks(row1 - row0);
    if (P < 1 || P > kGcMaxGroups || nb >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)nb), blk(kGcThreads);
    const int64_t npad = gc_npad(N);
#define GPCA_GC(PK, NB) hipLaunchKernelGGL((k_group_counts<PK, NB>), grid, blk, 0, st, G, ldr, krows, N, npad, O, size, P, row0, row1, counts, bad)
    if (gc_ppad(P) == 32) { if (packed) GPCA_GC(true, 1); else GPCA_GC(false, 1); }
    else { if (packed) GPCA_GC(true, 2); else GPCA_GC(false, 2); }
#undef GPCA_GC
    return 0;
}

}  // namespace gpca
