// KING-robust kinship (gpca_king, gpca_king.cpp): a lower-triangular symmetric rank-K update over the kept SNP rows.
//
// Per sample and kept row, three int8 indicators of the call g: H = [g == 1], M = [missing], X = g - 1 on homozygous calls (0 else).
// A pair (a, b) needs five integer sums over the kept rows: XX = sum X_a X_b, HH = sum H_a H_b, HM = sum H_a M_b, MH = sum M_a H_b and
// MM = sum M_a M_b; with the per-sample het and missing counts (k_king_vec) they give NSNP, the het counts of each sample over the rows
// where both are called, IBS0 and the kinship (k_king_finish; the identity is in include/gpca.h, section a9).
//
// Workgroup = one 128 x 128 tile (tile row >= tile column) of the output, 8 waves of 32 x 64 (the row side decoded once for both halves).  The genotypes go through LDS in stages
// of kKingStageRows rows, transposed to [sample][row] so that a lane reads its 16 k-contiguous bytes with one ds_read_b128.  Two LDS
// buffers: the waves multiply stage s from one while stage s + 1 (loaded into registers during stage s - 1) is written to the other and
// the global loads of stage s + 2 are issued, with one barrier per stage.  Each 32-row block of a stage costs two MFMAs (X X^T, H H^T);
// blocks where a wave ballot finds a missing call on a kept row add three (H M^T, M H^T, M M^T).  Rows that are not kept are zeroed in
// the row-side operands (and in the column side's M, for the ballot) from the call's kept-row bit mask.
// The sums are exact in i32 (K < 2^31) and are added to f64 running sums once per launch: the bits depend on nothing but the counts.
#include "syrk_tile.h"

namespace gpca {

constexpr int kKingThreads = 512;              // 8 waves: 4 x 2 strips of 32 x 64 (two 32 x 32 sub-tiles that share the row side)
constexpr int kKingStageRows = 64;             // rows per LDS stage (2 blocks of 32)
constexpr int kKingPitch = kKingStageRows + 16;  // bytes per sample of a staged side (ds_read_b128 stays 16-byte aligned)
constexpr int kKingUnits = 2 * kKingTile / 4 * kKingStageRows / 4 / kKingThreads;   // 4 x 4 (rows x samples) units per thread and stage
constexpr int kKingRQ = kKingStageRows / 4;       // row quads of a stage
static_assert(kKingUnits >= 1 && kKingRQ % 16 == 0 && (kKingRQ / 16 & (kKingRQ / 16 - 1)) == 0, "staging map");

// Unit q of a stage (q = threadIdx.x + kKingThreads * j): side = q / (32 kKingRQ), then kKingRQ row quads x 32 sample quads per side,
// laid out so that a wave covers 16 row quads x 4 sample quads (its LDS stores spread over the banks).
__device__ __forceinline__ void king_unit(int q, int& side, int& rq, int& cq) {
    constexpr int hi = kKingRQ / 16, hb = hi == 1 ? 0 : (hi == 2 ? 1 : 2);
    side = q / (32 * kKingRQ);
    const int u = q % (32 * kKingRQ);
    rq = (u & 15) | (((u >> 6) & (hi - 1)) << 4);
    cq = ((u >> 4) & 3) | ((u >> (6 + hb)) << 2);
}
struct KingFetch { unsigned x[kKingUnits][4]; };
template <bool PACKED>
__device__ __forceinline__ void king_fetch(KingFetch& F, const uint8_t* __restrict__ G, int64_t ldr, int64_t stage, int64_t ca0, int64_t cb0) {
#pragma unroll
    for (int j = 0; j < kKingUnits; ++j) {
        int side, rq, cq;
        king_unit((int)threadIdx.x + kKingThreads * j, side, rq, cq);
        const int64_t col = (side ? cb0 : ca0) + 4 * cq;
        unit_fetch<PACKED>(F.x[j], G + (stage * kKingStageRows + 4 * rq) * ldr + (PACKED ? col / 4 : col), ldr);
    }
}
template <bool PACKED>
__device__ __forceinline__ void king_put(const KingFetch& F, uint8_t* buf) {
#pragma unroll
    for (int j = 0; j < kKingUnits; ++j) {
        int side, rq, cq;
        king_unit((int)threadIdx.x + kKingThreads * j, side, rq, cq);
        unit_put<PACKED>(F.x[j], buf + (side * kKingTile + 4 * cq) * kKingPitch + 4 * rq, kKingPitch);
    }
}

// R [5][E]: f64 running sums XX, HH, HM, MH, MM of the band (E entries; first: they start at 0).  Band element (a, b < a),
// row0 <= a < row1, a < N, at band_index(row0, a, b, false); HM / MH: H / M of the row-side sample a.
template <bool PACKED>
__global__ __launch_bounds__(kKingThreads, 1) void k_king(const void* __restrict__ Gv, int64_t ldr, int64_t rows_pad,
                                                          const uint32_t* __restrict__ kmask, const int2* __restrict__ tiles, int64_t row0,
                                                          int64_t row1, int64_t N, double* __restrict__ R, int64_t E, int first) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[2][2 * kKingTile * kKingPitch];
    const uint8_t* G = (const uint8_t*)Gv;
    const int2 tl = tiles[blockIdx.x];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5, wa = wv >> 1, wb = 2 * (wv & 1);
    const int64_t ca0 = (int64_t)tl.x * kKingTile, cb0 = (int64_t)tl.y * kKingTile;
    // the wave's two sub-tiles (wa, wb + j); those above the diagonal of a diagonal tile are skipped
    const bool act0 = !(tl.x == tl.y && wb > wa), act1 = !(tl.x == tl.y && wb + 1 > wa);

    i32x16 xx[2], hh[2], hm[2], mh[2], mm[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) { xx[j][e] = 0; hh[j][e] = 0; hm[j][e] = 0; mh[j][e] = 0; mm[j][e] = 0; }
    const int64_t nblk = rows_pad >> 5;
    const int64_t nst = (nblk * 32 + kKingStageRows - 1) / kKingStageRows;
    const int a_off = (32 * wa + c) * kKingPitch, b_off = (kKingTile + 32 * wb + c) * kKingPitch;
    KingFetch F;
    king_fetch<PACKED>(F, G, ldr, 0, ca0, cb0);
    king_put<PACKED>(F, lds[0]);
    if (nst > 1) king_fetch<PACKED>(F, G, ldr, 1, ca0, cb0);
    __syncthreads();
    for (int64_t s = 0; s < nst; ++s) {
        const uint8_t* buf = lds[s & 1];
        if (act0) {
#pragma unroll
            for (int bi = 0; bi < kKingStageRows / 32; ++bi) {
                const int64_t blk = s * (kKingStageRows / 32) + bi;
                if (blk >= nblk) break;
                const unsigned km = (kmask[blk] >> (16 * h)) & 0xffffu;
                const i32x4 va = *reinterpret_cast<const i32x4*>(buf + a_off + 32 * bi + 16 * h);
                i32x4 XA, HA, MA, XB[2], HB[2], MB[2];
                unsigned anym = 0u;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned kb = kept_bytes(km, k);   // kept rows of these 4 bytes
                    const unsigned a = (unsigned)va[k];
                    const unsigned ma = (a >> 7) & 0x01010101u;
                    // X: hom = bit 0 clear (0 or 2; the missing code 0x81 has it set), two = bit 1 set (2 only)
                    const unsigned oa = ~a & 0x01010101u & kb, ta = (a >> 1) & 0x01010101u & kb;
                    XA[k] = (int)((oa * 0xffu) ^ (ta * 0xfeu));
                    HA[k] = (int)(a & ~ma & 0x01010101u & kb);
                    MA[k] = (int)(ma & kb);
                    anym |= ma & kb;
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const i32x4 vb = *reinterpret_cast<const i32x4*>(buf + b_off + 32 * j * kKingPitch + 32 * bi + 16 * h);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const unsigned kb = kept_bytes(km, k);
                        const unsigned b = (unsigned)vb[k];
                        const unsigned mb = (b >> 7) & 0x01010101u;
                        const unsigned ob = ~b & 0x01010101u, tb = (b >> 1) & 0x01010101u;
                        XB[j][k] = (int)((ob * 0xffu) ^ (tb * 0xfeu));
                        HB[j][k] = (int)(b & ~mb & 0x01010101u);
                        MB[j][k] = (int)(mb & kb);
                        anym |= mb & kb;
                    }
                }
                const bool miss = __builtin_amdgcn_ballot_w64(anym != 0u) != 0ull;   // wave-uniform
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (j == 1 && !act1) break;
                    xx[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(XA, XB[j], xx[j], 0, 0, 0);
                    hh[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(HA, HB[j], hh[j], 0, 0, 0);
                    if (miss) {
                        hm[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(HA, MB[j], hm[j], 0, 0, 0);
                        mh[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(MA, HB[j], mh[j], 0, 0, 0);
                        mm[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(MA, MB[j], mm[j], 0, 0, 0);
                    }
                }
            }
        }
        if (s + 1 < nst) king_put<PACKED>(F, lds[(s + 1) & 1]);     // (its last readers finished before the previous barrier)
        if (s + 2 < nst) king_fetch<PACKED>(F, G, ldr, s + 2, ca0, cb0);
        __syncthreads();
    }
    const int64_t a_base = ca0 + 32 * wa;
    const int64_t base = band_entries(0, row0, false);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int64_t b_col = cb0 + 32 * (wb + j) + c;
        if (!(j ? act1 : act0) || b_col >= N) continue;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int64_t a = acc_row(a_base, e, h);
            if (band_holds<false>(row0, row1, N, a, b_col)) {
                const int64_t ix = band_entries(0, a, false) - base + b_col;
                const double v[5] = {(double)xx[j][e], (double)hh[j][e], (double)hm[j][e], (double)mh[j][e], (double)mm[j][e]};
#pragma unroll
                for (int t = 0; t < 5; ++t) R[t * E + ix] = first ? v[t] : R[t * E + ix] + v[t];
            }
        }
    }
}

void launch_king(hipStream_t st, const void* G, int packed, int64_t ldr, int64_t rows_pad, const uint32_t* kmask, const int2* tiles,
                 int64_t ntiles, int64_t row0, int64_t row1, int64_t N, double* R, int64_t E, int first) {
    if (ntiles <= 0) return;
    if (packed) hipLaunchKernelGGL(k_king<true>, dim3((unsigned)ntiles), dim3(kKingThreads), 0, st, G, ldr, rows_pad, kmask, tiles, row0, row1, N, R, E, first);
    else hipLaunchKernelGGL(k_king<false>, dim3((unsigned)ntiles), dim3(kKingThreads), 0, st, G, ldr, rows_pad, kmask, tiles, row0, row1, N, R, E, first);
}

// Per sample n and group of kKingVecRows rows: het[n] += kept rows with g == 1, miss[n] += kept rows missing (u32 atomics on the call's
// own device buffers: exact in any order), bad |= 1 for a kept row holding a value outside {0, 1, 2, -127}.
constexpr int kKingVecRows = 4096;
template <bool PACKED>
__global__ __launch_bounds__(256) void k_king_vec(const void* __restrict__ Gv, int64_t ldr, int64_t rows, int64_t Npad,
                                                  const uint8_t* __restrict__ keep, unsigned* __restrict__ het, unsigned* __restrict__ miss,
                                                  unsigned* __restrict__ bad) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= Npad) return;
    const uint8_t* G = (const uint8_t*)Gv;
    const int64_t i0 = (int64_t)blockIdx.y * kKingVecRows, i1 = i0 + kKingVecRows < rows ? i0 + kKingVecRows : rows;
    unsigned nh = 0, nm = 0, bd = 0;
    for (int64_t i = i0; i < i1; ++i) {
        if (!keep[i]) continue;
        const unsigned v = call_at<PACKED>(G, ldr, i, n);
        if (v == kMissingByte) ++nm;
        else if (v == 1u) ++nh;
        else if (v != 0u && v != 2u) bd = 1u;
    }
    if (nh) atomicAdd(het + n, nh);
    if (nm) atomicAdd(miss + n, nm);
    if (bd) atomicOr(bad, 1u);
}
void launch_king_vec(hipStream_t st, const void* G, int packed, int64_t ldr, int64_t rows, int64_t Npad, const uint8_t* keep,
                     unsigned* het, unsigned* miss, unsigned* bad) {
    const int64_t ng = (rows + kKingVecRows - 1) / kKingVecRows;
    if (ng <= 0) return;
    const dim3 grid((unsigned)((Npad + 255) / 256), (unsigned)ng);
    if (packed) hipLaunchKernelGGL(k_king_vec<true>, grid, dim3(256), 0, st, G, ldr, rows, Npad, keep, het, miss, bad);
    else hipLaunchKernelGGL(k_king_vec<false>, grid, dim3(256), 0, st, G, ldr, rows, Npad, keep, het, miss, bad);
}

// het_f[n] = het[n], miss_f[n] = miss[n] as f64 (plain stores into the exchange buffer, which may be pinned host memory)
__global__ __launch_bounds__(256) void k_king_vec_f64(const unsigned* __restrict__ het, const unsigned* __restrict__ miss, int64_t Npad,
                                                      double* __restrict__ het_f, double* __restrict__ miss_f) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= Npad) return;
    het_f[n] = (double)het[n];
    miss_f[n] = (double)miss[n];
}
void launch_king_vec_f64(hipStream_t st, const unsigned* het, const unsigned* miss, int64_t Npad, double* het_f, double* miss_f) {
    hipLaunchKernelGGL(k_king_vec_f64, dim3((unsigned)((Npad + 255) / 256)), dim3(256), 0, st, het, miss, Npad, het_f, miss_f);
}

// The kinship of every pair of the band (one workgroup per band row) from the summed counts, in f64 on exact integers (all below 2^53):
//   NSNP = K - miss_a - miss_b + MM,  het_ab = het_a - HM,  het_ba = het_b - MH,  homhom = NSNP - het_ab - het_ba + HH,
//   IBS0 = (homhom - XX) / 2,  kinship = 0.5 - (4 IBS0 + het_ab + het_ba - 2 HH) / (4 min(het_ab, het_ba))  (NaN when the min is 0).
// counts (may be NULL): [E][3] = NSNP, HETHET, IBS0.
__global__ __launch_bounds__(256) void k_king_finish(const double* __restrict__ R, int64_t E, const double* __restrict__ het,
                                                     const double* __restrict__ miss, double K, int64_t row0, double* __restrict__ kin,
                                                     int* __restrict__ counts) {
    const int64_t a = row0 + blockIdx.x;
    const int64_t o = band_index(row0, a, 0, false);
    for (int64_t b = threadIdx.x; b < a; b += 256) {
        const int64_t ix = o + b;
        const double XX = R[ix], HH = R[E + ix], HM = R[2 * E + ix], MH = R[3 * E + ix], MM = R[4 * E + ix];
        const double nsnp = ((K - miss[a]) - miss[b]) + MM;
        const double het_ab = het[a] - HM, het_ba = het[b] - MH;
        const double homhom = ((nsnp - het_ab) - het_ba) + HH;
        const double ibs0 = (homhom - XX) * 0.5;
        const double mn = het_ab < het_ba ? het_ab : het_ba;
        const double num = ((4.0 * ibs0 + het_ab) + het_ba) - 2.0 * HH;
        kin[ix] = mn == 0.0 ? __builtin_nan("") : 0.5 - num / (4.0 * mn);
        if (counts) { counts[3 * ix] = (int)nsnp; counts[3 * ix + 1] = (int)HH; counts[3 * ix + 2] = (int)ibs0; }
    }
}
void launch_king_finish(hipStream_t st, const double* R, int64_t E, const double* het, const double* miss, double K, int64_t row0,
                        int64_t row1, double* kin, int* counts) {
    if (row1 <= row0) return;
    hipLaunchKernelGGL(k_king_finish, dim3((unsigned)(row1 - row0)), dim3(256), 0, st, R, E, het, miss, K, row0, kin, counts);
}

}  // namespace gpca
