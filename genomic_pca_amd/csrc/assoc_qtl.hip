// Many-trait QTL scan (gpca_assoc_qtl; gpca_assoc_qtl.cpp, include/gpca.h section a24): the regression of gpca_assoc_linear for every
// kept row against T <= 2^20 traits, of which only the pairs with r2 >= r2_min and the best row per trait leave the device.
//
// k_assoc_qtl: a workgroup owns kAscRows kept rows x a strip of tw trait columns (blockIdx.x = row block of the launch, blockIdx.y =
// strip) and walks the strip in tiles of kQtlTile = 64 columns.  Per tile it runs asc_pipeline (assoc_tile.h) on the tile's 64 rows of
// the trait panel, with asc_put as the stager: the tile, the stages, the exact products, the order of the samples and the 256-sample
// flush are k_assoc's with NB = 2, so d, e and xb = d + mbar e carry gpca_assoc_linear's bits whichever traits share the tile.  The
// calls of the 128 rows are staged again for every tile; after the first tile they come from L2 (128 x npad bytes per workgroup), HBM
// sees a row block once per strip.  The per-row pass before it (launch_assoc on the covariate basis, k_assoc_finish) leaves the sums
// and rowinfo = n_obs, a1_freq, xx, sxx, from which a thread per row forms mbar and liveness (n_obs != 0, xx > 0, not sxx max_vif < xx).
// Epilogue of a tile (f64, no contraction): r2 = (xb xb) / (sxx yy_t); hit = live and r2 >= r2_min.
//   records: per accumulator element a wave ballot, one 64-bit integer atomicAdd on the call's counter per ballot that found a hit, the
//     lanes write at base + their rank; a record at or past cap is dropped.  The counter ends at n_found in every case; the host sorts
//     the records by (row, trait), so no output depends on the order of the atomics.
//   hit_count: a row of the tile belongs to one lane half of one wave, which keeps its count in LDS (plain adds, one lane per row); one
//     integer atomicAdd per row and workgroup at the end (the strips of a row block share the row).
//   best: per tile the lanes reduce their 16 rows, the halves by a shuffle, the 4 waves through LDS; the workgroup's best (r2, row) of
//     every column goes to ws [row block][T] (r2 = -1, row = -1 without a live row).  k_assoc_qtl_best, a thread per trait, folds the
//     blocks of a launch in ascending order into the running best with a strict >, so the smallest row wins a tie.  No atomic on an output,
//     no float atomic anywhere.
// Registers: the pipeline's 2 x (2 x 16 f32 + 2 x 16 f64) sums as in k_assoc with lpad = 64, plus the epilogue's few f64 temporaries:
// the compiler takes 256 VGPRs + 136 AGPRs (int8 rows; 142 on 2-bit rows) of the 512 a wave of a 256-thread workgroup may use, no
// scratch and no VGPR spill (22 SGPRs go to VGPR lanes): one wave per SIMD.  LDS (static, qtl_lds_bytes): the two
// stage buffers of AscSmem<2, 3> = 54 784 B, mbar and sxx 2 x 1 KiB, live and the hit counts 2 x 512 B, the waves' bests 4 x 64 x 16 B
// = 4 KiB: 61 952 B of the 160 KiB.
// Out of scope (cis windows and permutations: assoc_qtl_cis.hip): per-trait sample sets, interaction terms, case / control traits,
// reduced-precision operands, streamed and row-sharded handles.
#include "assoc_tile.h"

#pragma clang fp contract(off)

namespace gpca {

struct QtlSmem {
    AscSmem<2, 3> asc;
    double mbar[kAscRows], sxx[kAscRows];
    unsigned live[kAscRows], hits[kAscRows];
    double wr2[4][kQtlTile];
    long long wrow[4][kQtlTile];
};
static_assert(sizeof(QtlSmem) == qtl_lds_bytes() && qtl_lds_bytes() <= 64 * 1024, "static LDS of k_assoc_qtl");

// Bt [qtl_tpad(T)][npad], yy [qtl_tpad(T)]; sums [rows][3], info [rows][4], hit_count [rows] of the band [band0, ...); the launch covers
// the kept rows [row0, row1), row0 - band0 a multiple of kAscRows; ws_r2 / ws_row [gridDim.x][T]; tiles_per_strip = tw / kQtlTile
template <bool PACKED>
__global__ __launch_bounds__(kAscThreads) void k_assoc_qtl(const void* __restrict__ Gv, int64_t ldr, const int64_t* __restrict__ krows, int64_t N,
                                                           int64_t npad, const float* __restrict__ Bt, const unsigned* __restrict__ incw,
                                                           const double* __restrict__ yy, int64_t T, int tiles_per_strip, int64_t band0,
                                                           int64_t row0, int64_t row1, const unsigned* __restrict__ sums,
                                                           const double* __restrict__ info, double max_vif, double r2_min,
                                                           unsigned* __restrict__ hit_count, unsigned* __restrict__ hit_index,
                                                           double* __restrict__ hit_value, unsigned long long cap,
                                                           unsigned long long* __restrict__ counter, double* __restrict__ ws_r2,
                                                           long long* __restrict__ ws_row) {
    __shared__ __attribute__((aligned(16))) QtlSmem sm;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int64_t k0 = row0 + (int64_t)blockIdx.x * kAscRows;
    const int srow = threadIdx.x >> 1;                                     // (the pipeline's staging map)
    const int64_t sorow = k0 + srow < row1 ? krows[k0 + srow] : -1;

    if (threadIdx.x < kAscRows) {
        const int r = threadIdx.x;
        const int64_t kr = k0 + r;
        double mbar = 0.0, sxx = 1.0;
        unsigned live = 0u;
        if (kr < row1) {
            const unsigned* s = sums + (kr - band0) * 3;
            const double* o = info + (kr - band0) * 4;
            const double xx = o[2];
            mbar = (double)s[1] / (double)s[0];
            sxx = o[3];
            live = (s[0] == 0u || !(xx > 0.0) || sxx * max_vif < xx) ? 0u : 1u;
        }
        sm.mbar[r] = mbar; sm.sxx[r] = sxx; sm.live[r] = live; sm.hits[r] = 0u;
    }
    // (the pipeline's first barrier orders these writes before the first epilogue)

    const int64_t tile0 = (int64_t)blockIdx.y * tiles_per_strip;
    const int64_t ntiles = qtl_tiles(T);
    for (int64_t tile = tile0; tile < tile0 + tiles_per_strip && tile < ntiles; ++tile) {
        unsigned nobs = 0u, s1 = 0u, s2 = 0u, bd = 0u;                       // (the per-row pass has counted and checked the calls)
        double rd[2][16], re[2][16];
        asc_pipeline<PACKED, 2, false>(sm.asc, (const uint8_t*)Gv, ldr, sorow, N, npad, Bt + tile * kQtlTile * npad, incw,
                             [&](const AscFetch& F, unsigned inb, unsigned inc, uint8_t* dst) { asc_put(F, inb, inc, dst, nobs, s1, s2, bd); }, rd, re, nullptr, wv, lane);
        double br2[2] = {-1.0, -1.0};
        long long brow[2] = {-1, -1};
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int r = asc_acc_row(wv, h, e);
            const int64_t kr = k0 + r;
            const bool rowok = kr < row1 && sm.live[r] != 0u;
            const double mbar = sm.mbar[r], sxx = sm.sxx[r];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int64_t col = tile * kQtlTile + 32 * j + c;
                const double xb = rd[j][e] + mbar * re[j][e];
                const double r2 = (xb * xb) / (sxx * yy[col]);
                const bool ok = rowok && col < T;
                if (ok && (r2 > br2[j] || (r2 == br2[j] && kr < brow[j]))) { br2[j] = r2; brow[j] = kr; }
                const bool hit = ok && r2 >= r2_min;
                const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);                   // wave-uniform
                if (m != 0ull) {
                    unsigned long long base = 0ull;
                    if (lane == 0) base = atomicAdd(counter, (unsigned long long)__builtin_popcountll(m));
                    base = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(base >> 32)) << 32) |
                           (unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)base);
                    const unsigned long long at = base + (unsigned long long)__builtin_popcountll(m & ((1ull << lane) - 1ull));
                    if (hit && at < cap) {
                        hit_index[2 * at] = (unsigned)kr; hit_index[2 * at + 1] = (unsigned)col;
                        hit_value[2 * at] = xb; hit_value[2 * at + 1] = r2;
                    }
                    // (row r belongs to this lane half of this wave alone: a plain add by its lane c = 0)
                    if (c == 0) sm.hits[r] += (unsigned)__builtin_popcountll(h ? (m >> 32) : (m & 0xffffffffull));
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const double o2 = __shfl_xor(br2[j], 32);
            const long long orow = __shfl_xor(brow[j], 32);
            if (o2 > br2[j] || (o2 == br2[j] && orow >= 0 && orow < brow[j])) { br2[j] = o2; brow[j] = orow; }
            if (h == 0) { sm.wr2[wv][32 * j + c] = br2[j]; sm.wrow[wv][32 * j + c] = brow[j]; }
        }
        __syncthreads();
        if (threadIdx.x < kQtlTile) {
            const int64_t col = tile * kQtlTile + threadIdx.x;
            double b2 = sm.wr2[0][threadIdx.x];
            long long bw = sm.wrow[0][threadIdx.x];
            for (int w = 1; w < 4; ++w) {
                const double o2 = sm.wr2[w][threadIdx.x];
                const long long orow = sm.wrow[w][threadIdx.x];
                if (o2 > b2 || (o2 == b2 && orow >= 0 && orow < bw)) { b2 = o2; bw = orow; }
            }
            if (col < T) { ws_r2[qtl_wsbest_index(blockIdx.x, T, col)] = b2; ws_row[qtl_wsbest_index(blockIdx.x, T, col)] = bw; }
        }
        // (the next tile's pipeline passes a barrier before any wave reaches its epilogue and writes wr2 / wrow again)
    }
    __syncthreads();
    if (threadIdx.x < kAscRows && k0 + threadIdx.x < row1 && sm.hits[threadIdx.x] != 0u)
        atomicAdd(hit_count + (k0 + threadIdx.x - band0), sm.hits[threadIdx.x]);
}

int launch_assoc_qtl(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t N, const float* Bt,
                     const unsigned* incw, const double* yy, int64_t T, int tw, int64_t band0, int64_t row0, int64_t row1, const unsigned* sums,
                     const double* info, double max_vif, double r2_min, unsigned* hit_count, unsigned* hit_index, double* hit_value, int64_t cap,
                     unsigned long long* counter, double* ws_r2, long long* ws_row) {
    if (row1 <= row0) return 0;
    const int64_t nb = asc_row_blocks(row1 - row0), strips = qtl_strips(T, tw);
    if (T < 1 || T > kQtlMaxTraits || tw != qtl_clamp_tw(tw) || (row0 - band0) % kAscRows != 0 || row0 < band0 || cap < 0 ||
        nb > qtl_chunk_blocks(T) || nb >= ((int64_t)1 << 31) || strips > 65535)
        return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)nb, (unsigned)strips), blk(kAscThreads);
    const int64_t npad = asc_npad(N);
#define GPCA_QTL(PK) hipLaunchKernelGGL((k_assoc_qtl<PK>), grid, blk, 0, st, G, ldr, krows, N, npad, Bt, incw, yy, T, tw / kQtlTile, band0, row0, row1, \
                                        sums, info, max_vif, r2_min, hit_count, hit_index, hit_value, (unsigned long long)cap, counter, ws_r2, ws_row)
    if (packed) GPCA_QTL(true); else GPCA_QTL(false);
#undef GPCA_QTL
    return 0;
}

// a thread per trait: folds ws [blocks][T] into best [T] (r2 = -1, row = -1: none yet), blocks ascending, a strict >
__global__ __launch_bounds__(kQtlReduceThreads) void k_assoc_qtl_best(const double* __restrict__ ws_r2, const long long* __restrict__ ws_row,
                                                                      int64_t blocks, int64_t T, double* __restrict__ best_r2,
                                                                      long long* __restrict__ best_row) {
    const int64_t t = (int64_t)blockIdx.x * kQtlReduceThreads + threadIdx.x;
    if (t >= T) return;
    double b2 = best_r2[t];
    long long bw = best_row[t];
    for (int64_t b = 0; b < blocks; ++b) {
        const double o2 = ws_r2[qtl_wsbest_index(b, T, t)];
        if (o2 > b2) { b2 = o2; bw = ws_row[qtl_wsbest_index(b, T, t)]; }
    }
    best_r2[t] = b2; best_row[t] = bw;
}
void launch_assoc_qtl_best(hipStream_t st, const double* ws_r2, const long long* ws_row, int64_t blocks, int64_t T, double* best_r2,
                           long long* best_row) {
    if (blocks <= 0 || T <= 0) return;
    hipLaunchKernelGGL(k_assoc_qtl_best, dim3((unsigned)((T + kQtlReduceThreads - 1) / kQtlReduceThreads)), dim3(kQtlReduceThreads), 0, st,
                       ws_r2, ws_row, blocks, T, best_r2, best_row);
}

}  // namespace gpca
