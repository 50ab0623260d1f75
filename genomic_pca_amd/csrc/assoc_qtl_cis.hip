// cis-QTL mapping (gpca_assoc_qtl_cis, gpca_qtl_perm_panel; gpca_assoc_qtl_cis.cpp, include/gpca.h section a25): for one trait at a time, the
// best r2 over the kept rows of its window for the residual (column 0) and for P permutations of it (columns 1 .. P).
//
// k_qtl_perm_panel builds the trait's panel [qtl_tpad(P + 1)][npad] f32 in the layout asc_design_rows produces (the caller zeroes the
// buffer once: excluded samples, pad samples and pad columns are never written).  A workgroup owns qtl_perm_group(Pc) columns.  b_t (f64,
// the included samples in ascending order) sits in LDS when n <= kQtlPermLdsSamples and is gathered through the table, v_i = b[perm[p][i]].
//   step 1, a thread per (column, covariate j): c_j = sum_i Q_ij v_i, i ascending, one running sum -> LDS; Q reaches the threads through
//     LDS in tiles of kQtlPermQTile samples (pitch kQtlPermQPitch: the rows of the covariates fall on different banks);
//   step 2, the threads walk the samples of one column after the other: s_i = sum_j Q_ij c_j, j ascending, one running sum; the value is
//     (float)(v_i - s_i), written at the sample's place S[i].  Column 0 is (float) b_i; with Pc = 0 a permuted column is (float) v_i.
// All of it in f64 with contraction off: a product is rounded before it is added, so the order above fixes every bit and no bit depends
// on how the threads are mapped.  Q is [Pc][n], so both steps read it coalesced; the threads of a column share perm's row.
//
// k_assoc_qtl_cis<PACKED> is k_assoc_qtl's mainloop (asc_pipeline with asc_put: the same tile, stages, sample order and 256-sample flush,
// so xb carries gpca_assoc_linear's bits) on the row blocks that start at the window's lo, rows at and past hi clipped, with the
// best-per-column reduction as its only epilogue: no records, no counter, no hit counts, no atomic of any kind.  yy is the trait's yy_t
// for every column (a kernel argument).  The workgroup's best (r2, row) of every column goes to ws [row block][P + 1] as in a24, and xb of
// column 0's best row to ws_xb [row block] (written by the strip that holds column 0).  k_assoc_qtl_cis_best, a thread per column, folds the
// row blocks of a launch in ascending order with a strict > into the running best of the trait; on the window's last launch it writes
// the results: perm_r2 [g][P] and column 0's (r2, xb, row).
// Out of scope: conditional passes, per-trait sample sets, interaction terms, streamed and row-sharded handles.
#include "assoc_tile.h"

#pragma clang fp contract(off)

namespace gpca {

__global__ __launch_bounds__(kQtlPermThreads) void k_qtl_perm_panel(const double* __restrict__ b, const double* __restrict__ Qt, int Pc, int64_t n,
                                                                    const uint32_t* __restrict__ perm, int64_t P, const int* __restrict__ S,
                                                                    int64_t npad, float* __restrict__ out) {
    __shared__ double sb[kQtlPermLdsSamples];
    __shared__ double sc[kQtlPermThreads];
    __shared__ double sq[kQtlMaxPc * kQtlPermQPitch];
    const bool inlds = n <= kQtlPermLdsSamples;                              // (uniform)
    if (inlds)
        for (int64_t i = threadIdx.x; i < n; i += kQtlPermThreads) sb[i] = b[i];
    __syncthreads();
    const int grp = qtl_perm_group(Pc);
    const int64_t col0 = (int64_t)blockIdx.x * grp;
    if (Pc > 0) {
        const int cl = (int)threadIdx.x / Pc, j = (int)threadIdx.x - cl * Pc;
        const int64_t col = col0 + cl;
        const bool mine = cl < grp && col >= 1 && col <= P;
        const uint32_t* pr = perm + (mine ? col - 1 : 0) * n;
        const double* qrow = sq + j * kQtlPermQPitch;
        double c = 0.0;
        // Q goes through LDS in tiles of kQtlPermQTile samples, read coalesced once per workgroup; a thread adds its tile's terms in
        // ascending i, so the sum keeps its order across the tiles
        for (int64_t i0 = 0; i0 < n; i0 += kQtlPermQTile) {
            __syncthreads();                                                 // (the tile before has been read)
            for (int k = threadIdx.x; k < Pc * kQtlPermQTile; k += kQtlPermThreads) {
                const int jj = k / kQtlPermQTile, ii = k - jj * kQtlPermQTile;
                sq[jj * kQtlPermQPitch + ii] = i0 + ii < n ? Qt[(int64_t)jj * n + i0 + ii] : 0.0;
            }
            __syncthreads();
            if (mine) {
                const int m = n - i0 < kQtlPermQTile ? (int)(n - i0) : kQtlPermQTile;
                if (m == kQtlPermQTile) {
#pragma unroll 8
                    for (int u = 0; u < kQtlPermQTile; ++u) { const uint32_t s = pr[i0 + u]; c += qrow[u] * (inlds ? sb[s] : b[s]); }
                } else {
                    for (int u = 0; u < m; ++u) { const uint32_t s = pr[i0 + u]; c += qrow[u] * (inlds ? sb[s] : b[s]); }
                }
            }
        }
        if (mine) sc[cl * Pc + j] = c;
        __syncthreads();
    }
    for (int cl = 0; cl < grp; ++cl) {
        const int64_t col = col0 + cl;
        if (col > P) break;
        const uint32_t* pr = col > 0 ? perm + (col - 1) * n : nullptr;
        for (int64_t i = threadIdx.x; i < n; i += kQtlPermThreads) {
            const int64_t src = pr ? (int64_t)pr[i] : i;
            const double v = inlds ? sb[src] : b[src];
            double val = v;
            if (pr && Pc > 0) {
                double s = 0.0;
                for (int j = 0; j < Pc; ++j) s += Qt[(int64_t)j * n + i] * sc[cl * Pc + j];
                val = v - s;
            }
            out[qtl_cis_panel_index(col, npad, S ? (int64_t)S[i] : i)] = (float)val;
        }
    }
}

void launch_qtl_perm_panel(hipStream_t st, const double* b, const double* Qt, int Pc, int64_t n, const uint32_t* perm, int64_t P, const int* S,
                           int64_t npad, float* out) {
    if (n <= 0 || P < 0) return;
    hipLaunchKernelGGL(k_qtl_perm_panel, dim3((unsigned)qtl_perm_grid(P, Pc)), dim3(kQtlPermThreads), 0, st, b, Qt, Pc, n, perm, P, S, npad, out);
}

struct QtlCisSmem {
    AscSmem<2, 3> asc;
    double mbar[kAscRows], sxx[kAscRows];
    unsigned live[kAscRows];
    double wr2[4][kQtlTile];
    long long wrow[4][kQtlTile];
    double wxb[4];
};
static_assert(sizeof(QtlCisSmem) == qtl_cis_lds_bytes(), "static LDS of k_assoc_qtl_cis");

// Bt [qtl_tpad(T)][npad]; sums [rows][3], info [rows][4] of the per-row pass over the band [band0, ...); the launch covers the kept rows
// [row0, row1) (row0 = the window's lo plus whole row blocks, row1 = the launch's end, at most hi); ws_r2 / ws_row [gridDim.x][T],
// ws_xb [gridDim.x]; tiles_per_strip = tw / kQtlTile
template <bool PACKED>
__global__ __launch_bounds__(kAscThreads) void k_assoc_qtl_cis(const void* __restrict__ Gv, int64_t ldr, const int64_t* __restrict__ krows, int64_t N,
                                                               int64_t npad, const float* __restrict__ Bt, const unsigned* __restrict__ incw,
                                                               double yy, int64_t T, int tiles_per_strip, int64_t band0, int64_t row0,
                                                               int64_t row1, const unsigned* __restrict__ sums, const double* __restrict__ info,
                                                               double max_vif, double* __restrict__ ws_r2, long long* __restrict__ ws_row,
                                                               double* __restrict__ ws_xb) {
    __shared__ __attribute__((aligned(16))) QtlCisSmem sm;
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
        sm.mbar[r] = mbar; sm.sxx[r] = sxx; sm.live[r] = live;
    }
    // (the pipeline's first barrier orders these writes before the first epilogue)

    const int64_t tile0 = (int64_t)blockIdx.y * tiles_per_strip;
    const int64_t ntiles = qtl_tiles(T);
    for (int64_t tile = tile0; tile < tile0 + tiles_per_strip && tile < ntiles; ++tile) {
        unsigned nobs = 0u, s1 = 0u, s2 = 0u, bd = 0u;                       // (the per-row pass has counted and checked the calls)
        double rd[2][16], re[2][16];
        asc_pipeline<PACKED, 2, false>(sm.asc, (const uint8_t*)Gv, ldr, sorow, N, npad, Bt + tile * kQtlTile * npad, incw,
                             [&](const AscFetch& F, unsigned inb, unsigned inc, uint8_t* dst) { asc_put(F, inb, inc, dst, nobs, s1, s2, bd); }, rd, re, nullptr, wv, lane);
        double br2[2] = {-1.0, -1.0}, bxb = 0.0;                             // bxb: xb of (br2[0], brow[0])
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
                const double r2 = (xb * xb) / (sxx * yy);
                const bool ok = rowok && col < T;
                if (ok && (r2 > br2[j] || (r2 == br2[j] && kr < brow[j]))) {
                    br2[j] = r2; brow[j] = kr;
                    if (j == 0) bxb = xb;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const double o2 = __shfl_xor(br2[j], 32);
            const long long orow = __shfl_xor(brow[j], 32);
            const double oxb = __shfl_xor(bxb, 32);
            if (o2 > br2[j] || (o2 == br2[j] && orow >= 0 && orow < brow[j])) {
                br2[j] = o2; brow[j] = orow;
                if (j == 0) bxb = oxb;
            }
            if (h == 0) { sm.wr2[wv][32 * j + c] = br2[j]; sm.wrow[wv][32 * j + c] = brow[j]; }
        }
        if (lane == 0) sm.wxb[wv] = bxb;                                     // (column 32 j + c = 0 of the tile; read for tile 0 only)
        __syncthreads();
        if (threadIdx.x < kQtlTile) {
            const int64_t col = tile * kQtlTile + threadIdx.x;
            double b2 = sm.wr2[0][threadIdx.x];
            long long bw = sm.wrow[0][threadIdx.x];
            double bx = sm.wxb[0];
            for (int w = 1; w < 4; ++w) {
                const double o2 = sm.wr2[w][threadIdx.x];
                const long long orow = sm.wrow[w][threadIdx.x];
                if (o2 > b2 || (o2 == b2 && orow >= 0 && orow < bw)) { b2 = o2; bw = orow; bx = sm.wxb[w]; }
            }
            if (col < T) { ws_r2[qtl_wsbest_index(blockIdx.x, T, col)] = b2; ws_row[qtl_wsbest_index(blockIdx.x, T, col)] = bw; }
            if (col == 0) ws_xb[blockIdx.x] = bx;
        }
        // (the next tile's pipeline passes a barrier before any wave reaches its epilogue and writes wr2 / wrow / wxb again)
    }
}

int launch_assoc_qtl_cis(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t N, const float* Bt,
                         const unsigned* incw, double yy, int64_t T, int tw, int64_t band0, int64_t row0, int64_t row1, const unsigned* sums,
                         const double* info, double max_vif, double* ws_r2, long long* ws_row, double* ws_xb) {
    if (row1 <= row0) return 0;
    const int64_t nb = asc_row_blocks(row1 - row0), strips = qtl_strips(T, tw);
    if (T < 1 || T > kQtlCisMaxPerm + 1 || tw != qtl_clamp_tw(tw) || row0 < band0 || nb > qtl_chunk_blocks(T) || nb >= ((int64_t)1 << 31) ||
        strips > 65535)
        return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)nb, (unsigned)strips), blk(kAscThreads);
    const int64_t npad = asc_npad(N);
#define GPCA_QTL_CIS(PK) hipLaunchKernelGGL((k_assoc_qtl_cis<PK>), grid, blk, 0, st, G, ldr, krows, N, npad, Bt, incw, yy, T, tw / kQtlTile, band0, \
                                            row0, row1, sums, info, max_vif, ws_r2, ws_row, ws_xb)
    if (packed) GPCA_QTL_CIS(true); else GPCA_QTL_CIS(false);
#undef GPCA_QTL_CIS
    return 0;
}

// a thread per column: folds ws [blocks][T] into run [T] (first: starts from r2 = -1, row = -1), blocks ascending, a strict >; last: the
// results of trait g: perm_r2 [g][P] (NaN without a live row) and best [g][3] = r2, xb, row of column 0
__global__ __launch_bounds__(kQtlReduceThreads) void k_assoc_qtl_cis_best(const double* __restrict__ ws_r2, const long long* __restrict__ ws_row,
                                                                          const double* __restrict__ ws_xb, int64_t blocks, int64_t T, int first,
                                                                          int last, double* __restrict__ run_r2, long long* __restrict__ run_row,
                                                                          double* __restrict__ run_xb, int64_t g, double* __restrict__ perm_r2,
                                                                          double* __restrict__ best) {
    const int64_t t = (int64_t)blockIdx.x * kQtlReduceThreads + threadIdx.x;
    if (t >= T) return;
    double b2 = first ? -1.0 : run_r2[t], bx = (t == 0 && !first) ? run_xb[0] : 0.0;
    long long bw = first ? -1 : run_row[t];
    for (int64_t b = 0; b < blocks; ++b) {
        const double o2 = ws_r2[qtl_wsbest_index(b, T, t)];
        if (o2 > b2) {
            b2 = o2; bw = ws_row[qtl_wsbest_index(b, T, t)];
            if (t == 0) bx = ws_xb[b];
        }
    }
    if (!last) {
        run_r2[t] = b2; run_row[t] = bw;
        if (t == 0) run_xb[0] = bx;
        return;
    }
    const double nan = __builtin_nan("");
    if (t == 0) { best[3 * g] = bw < 0 ? nan : b2; best[3 * g + 1] = bw < 0 ? nan : bx; best[3 * g + 2] = (double)bw; }
    else perm_r2[qtl_cis_result_index(g, T - 1, t - 1)] = bw < 0 ? nan : b2;
}
void launch_assoc_qtl_cis_best(hipStream_t st, const double* ws_r2, const long long* ws_row, const double* ws_xb, int64_t blocks, int64_t T,
                               int first, int last, double* run_r2, long long* run_row, double* run_xb, int64_t g, double* perm_r2, double* best) {
    if (blocks <= 0 || T <= 0) return;
    hipLaunchKernelGGL(k_assoc_qtl_cis_best, dim3((unsigned)((T + kQtlReduceThreads - 1) / kQtlReduceThreads)), dim3(kQtlReduceThreads), 0, st,
                       ws_r2, ws_row, ws_xb, blocks, T, first, last, run_r2, run_row, run_xb, g, perm_r2, best);
}

}  // namespace gpca
