// Host arithmetic that sizes launches and workspaces: part counts, slice counts, GEMM plans, and the capacity of every buffer they
// write.  Plain C++ (no HIP type): kernels.h includes it for the engine, tests/cpp/plan_audit.cpp includes it under a host compiler
// and checks every writer's extent against the capacity of the buffer it writes.  A buffer's size is stated here ONCE, as a function
// that its allocation site and the audit both call.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <initializer_list>
#include <vector>

namespace gpca {

// Row pitch of the int8 genotype matrix and row count of Q/Y buffers: multiple of this many samples.
constexpr int64_t kSamplePad = 256;   // = samples covered by one wave tile of the G^T T kernel
constexpr int kGQRowsPerWave = 128;   // SNP rows per wave in the G Q kernel (R = 4 tiles of 32)
constexpr int kMaxSketchCols = 128;   // = kMaxSketch (gpca_internal.h)

// ---- part counts of the tall-skinny helpers (kernels.hip, fold_quantize_i8.hip) --------------------------------------------------
// sketch operand: cpart[wave][j], one wave per 64 rows
inline int64_t omega_num_parts(int64_t Mpad) { return (Mpad + 63) / 64; }

// slices of the part axis in stage 1 of the two-stage sum.  Few elements per part (E <= 64: the c = b^T T partials, one per 32-row unit,
// 31 250 of them at a million SNPs) put a single column of workgroups on the grid: up to 256 slices there instead of 64 (14 us -> ~5 us
// for 4 MB).  S depends on (P, E) only, so the summation tree -- and with it every bit of the result -- is the same for every run and partition.
constexpr int kSumSlicesMax = 64, kSumSlicesMaxNarrow = 256;      // what a consumer that folds the slices itself must hold (narrow: E <= 64)
inline int sum_slices(int64_t P, int64_t E) {
    const int64_t cap = E <= 64 ? kSumSlicesMaxNarrow : kSumSlicesMax;
    int64_t s = (P + 63) / 64;
    return (int)(s < 1 ? 1 : (s > cap ? cap : s));
}
// doubles the first stage of a sum of parts of [E] writes at most, whatever the part count
inline int64_t sum_scratch_need(int64_t E) { return (E <= 64 ? (int64_t)kSumSlicesMaxNarrow : (int64_t)kSumSlicesMax) * E; }
// doubles of scratch per 32-column block of the sketch that launch_post_k1 / launch_quantize_f32_cfold use (<= 256 slices x 32 columns)
constexpr int64_t kPostK1Scratch = 256 * 32;
inline int post_k1_slices(int64_t units) { return sum_slices(units, 32); }
// Capacity (doubles) of the scratch of a handle whose sums have at most Lmax * Lmax elements per part (the l x l Grams) and whose
// launch_post_k1 takes one kPostK1Scratch block per 32 columns: every slice count sum_slices can return fits, at any part count.
inline int64_t sum_scratch_capacity(int Lmax) {
    const int64_t E = (int64_t)Lmax * Lmax;
    const int64_t need = std::max(sum_scratch_need(64), sum_scratch_need(E));      // (64 E grows with E above 64; 256 E tops at E = 64)
    return std::max<int64_t>(need, (int64_t)(Lmax / 32) * kPostK1Scratch);
}

// Gram: rows per block adapt to the problem so that ~1024 blocks are in flight (N = 10^4 used to get 20 blocks).
inline int64_t gram_rows_per_block(int64_t rows) {
    // The sample-side Grams of CholeskyQR (N rows, four per call) sit on the critical path between two GEMM passes, and their partial
    // sums are folded by the ONE workgroup that factors the result (k_chol_inv_fold32): 32 parts up to 8k rows, rising to at most 64, which
    // one k_sum_partials launch still finishes (the matrix-core Gram of 10 000 x 32 takes 5 us with 63 workgroups, 11 with 16).
    if (rows <= 262144) {
        int64_t parts = rows / 256;
        parts = parts < 32 ? 32 : (parts > 64 ? 64 : parts);
        const int64_t q = (rows + parts - 1) / parts;
        return q < 32 ? 32 : (q + 31) / 32 * 32;
    }
    int64_t r = (rows + 1023) / 1024;
    r = (r + 31) / 32 * 32;
    return r < 32 ? 32 : (r > 2048 ? 2048 : r);
}
inline int64_t gram_num_parts(int64_t rows) { const int64_t rpb = gram_rows_per_block(rows); return (rows + rpb - 1) / rpb; }
// An upper bound of gram_num_parts over EVERY row count up to `rows` (the part count is not monotone in the rows: 294 912 rows make
// 1 024 parts, 294 913 make 922): what a buffer must hold when the same handle also folds Grams of fewer rows (the condensed features
// of gpca_rsvd_condensed, R <= M).
inline int64_t gram_max_parts(int64_t rows) {
    if (rows <= 262144) return 64;
    return std::max<int64_t>(1024, (rows + 2047) / 2048);
}

constexpr int kTailRows = 64;                       // rows per workgroup of the last right-multiplication of CholeskyQR2
inline int64_t tail_num_parts(int64_t rows_pad) { return (rows_pad + kTailRows - 1) / kTailRows; }
constexpr int64_t kFinishQFoldMax = 512;            // most tail partials that k_quantize<double> folds by itself

constexpr int kScoreParts = 48;                     // (x 64 columns x 16 B of candidates = 48 KiB of LDS in k_scores_sign)
inline int64_t scores_num_parts(int64_t rows) { const int64_t c = (rows + 255) / 256; return c < kScoreParts ? (c < 1 ? 1 : c) : kScoreParts; }
constexpr int kColsumRowsPerBlock = 256;
inline int64_t colsum_num_parts(int64_t rows) { return (rows + kColsumRowsPerBlock - 1) / kColsumRowsPerBlock; }
constexpr int kAbsmaxRowsPerBlock = 1024;
inline int64_t absmax_num_parts(int64_t rows) { return (rows + kAbsmaxRowsPerBlock - 1) / kAbsmaxRowsPerBlock; }

// ---- GEMM plans ------------------------------------------------------------------------------------------------------------------
// K1: 32-row units of the padded matrix; resident waves (multiple of 4), wave w owns a contiguous, balanced range of units
struct GqPlan { int64_t units; int64_t waves; };
inline GqPlan gq_plan(int64_t Mpad, int waves_target) {
    GqPlan p;
    p.units = Mpad / 32;
    int64_t w = waves_target < 4 ? 4 : waves_target;
    if (w > p.units) w = p.units;
    w = (w + 3) / 4 * 4;
    p.waves = w;
    return p;
}
// K2 (f32): a wave owns one 256-sample block and a contiguous range of SNP rows
struct GttPlan { int64_t nblocks_n; int W; int64_t rows_per_wave; int64_t grid; };
inline GttPlan gtt_plan(int64_t Mpad, int64_t Npad, int L, int target_waves) {
    GttPlan p;
    p.nblocks_n = Npad / kSamplePad;
    int64_t W = target_waves / p.nblocks_n;
    if (W < 1) W = 1;
    const int64_t maxW = Mpad / 32;
    if (W > maxW) W = maxW;
    int64_t rpw = (Mpad + W - 1) / W;
    rpw = (rpw + 31) / 32 * 32;          // even number of 16-row groups per wave (Mpad is a multiple of 128)
    W = (Mpad + rpw - 1) / rpw;
    p.W = (int)W;
    p.rows_per_wave = rpw;
    const int64_t ngroups = (p.nblocks_n + 3) / 4;
    p.grid = ngroups * W;
    (void)L;
    return p;
}
// K2 (exact path) work decomposition: see kernels.h
struct Gtt8Plan { int64_t nblocks_n; int W; int64_t rows_per_wave; int64_t grid; int tasks_per_wg; int64_t S; int64_t ngroups; int strided; int64_t C; };
inline Gtt8Plan gtt8_plan(int64_t Mpad, int64_t Npad, int target_waves) {
    Gtt8Plan p{};
    p.nblocks_n = Npad / 128;
    int64_t W = target_waves / p.nblocks_n;
    if (W < 1) W = 1;
    // a slice's digit-plane sums live in i32 accumulators: |g| <= 2 times |digit| <= 128 per row keeps 2^22 rows a factor 2 inside
    // 2^31 (only a resident matrix of > 4M rows AND > 260k samples would get there: more than one GPU holds)
    const int64_t minW = (Mpad + ((int64_t)1 << 22) - 1) >> 22;
    if (W < minW) W = minW;
    const int64_t maxW = Mpad / 128;
    if (W > maxW) W = maxW;
    int64_t rpw = (Mpad + W - 1) / W;
    rpw = (rpw + 127) / 128 * 128;       // k-blocks per wave: multiple of 4 (Mpad is a multiple of 128)
    W = (Mpad + rpw - 1) / rpw;
    p.W = (int)W;
    p.rows_per_wave = rpw;
    p.grid = ((p.nblocks_n + 3) / 4) * W;
    return p;
}
// several consecutive (row chunk, n-group) tasks per workgroup (kernels.h): W row chunks such that one batch of `grid0` workgroups
// covers the tasks evenly.  Cost model per candidate W, relative to the bytes of one sweep: batch fill (tasks rounded up to whole
// workgroup loads), ~3 stages of prologue / drain / tile store per task, the fold's read of W partial tiles, and 2 % when a row chunk's
// T' planes (16 KiB per stage) outgrow the share of an XCD's L2 they can expect to keep.
inline Gtt8Plan gtt8_plan_batched(int64_t Mpad, int64_t Npad, int target_waves) {
    Gtt8Plan p{};
    p.nblocks_n = Npad / 128;
    p.ngroups = (p.nblocks_n + 3) / 4;
    p.S = Mpad / 128;
    int64_t grid0 = target_waves / 8;                // the default target (2 048) = 256 workgroups = one per CU of an MI355X
    if (grid0 < 1) grid0 = 1;
    // a task's digit-plane sums live in i32 accumulators: at most 2^22 rows (32 768 stages) per task
    const int64_t wmin = std::max<int64_t>(1, (p.S + 32767) / 32768), wmax = std::min<int64_t>(p.S, 1024);
    double best = 1e300;
    int64_t bestW = wmin;
    for (int64_t W = wmin; W <= std::max(wmin, wmax); ++W) {
        const int64_t T = W * p.ngroups, k = (T + grid0 - 1) / grid0;
        double f = (double)(k * grid0) / (double)T;                                      // batch fill: k tasks per workgroup against T / grid0
        f *= 1.0 + 3.0 * (double)W / (double)p.S;                                        // per-task prologue / drain / store
        f += (double)W * 256.0 / (double)Mpad;                                           // the fold reads W x Npad x 256 B against Mpad x Npad
        if ((double)p.S / (double)W * 16384.0 > 3.0 * 1048576.0) f += 0.02;               // T' planes of a row chunk vs L2
        if (f < best - 1e-12) { best = f; bestW = W; }
    }
    p.C = (p.S + bestW - 1) / bestW;                  // stages per row chunk (the last chunk may be shorter)
    p.W = (int)((p.S + p.C - 1) / p.C);
    const int64_t T = (int64_t)p.W * p.ngroups;
    p.tasks_per_wg = (int)((T + grid0 - 1) / grid0);
    p.grid = (T + p.tasks_per_wg - 1) / p.tasks_per_wg;
    p.strided = 1;
    p.rows_per_wave = p.C * 128;                      // rows of a full task
    return p;
}
// K2 for at most 256 samples (int8 rows): every wave owns a row chunk of its own
constexpr int64_t kNarrowSamples = 256;
inline Gtt8Plan gtt8_plan_narrow(int64_t Mpad, int64_t N, int target_waves) {
    Gtt8Plan p{};
    p.nblocks_n = (N + 127) / 128;                      // 128-sample blocks that hold samples: 1 or 2
    int64_t W = target_waves / p.nblocks_n;
    if (W < 1) W = 1;
    const int64_t maxW = Mpad / 128;
    if (W > maxW) W = maxW;
    int64_t rpw = (Mpad + W - 1) / W;
    rpw = (rpw + 127) / 128 * 128;
    W = (Mpad + rpw - 1) / rpw;
    p.W = (int)W;
    p.rows_per_wave = rpw;
    p.grid = (W * p.nblocks_n + 3) / 4;
    return p;
}
// projection sweep (project.hip): n-groups of 4 x 64 samples, W row chunks
struct PrjPlan { int64_t ngroups; int W; int64_t rows_per_wave; int64_t grid; };
inline PrjPlan prj_plan(int64_t Mpad, int64_t Npad, int target_waves) {
    PrjPlan p{};
    const int64_t nblocks = Npad / 64;
    p.ngroups = (nblocks + 3) / 4;
    int64_t W = target_waves / nblocks;
    if (W < 1) W = 1;
    const int64_t minW = (Mpad + ((int64_t)1 << 22) - 1) >> 22;    // i32 accumulators: |g| |digit| <= 128 per row, 2^22 rows per wave at most
    if (W < minW) W = minW;
    const int64_t maxW = Mpad / 128;
    if (W > maxW) W = maxW;
    if (W < 1) W = 1;
    int64_t rpw = (Mpad + W - 1) / W;
    rpw = (rpw + 127) / 128 * 128;
    W = (Mpad + rpw - 1) / rpw;
    p.W = (int)W;
    p.rows_per_wave = rpw;
    p.grid = p.ngroups * W;
    return p;
}

// ---- workspace capacities (elements) ---------------------------------------------------------------------------------------------
// d_part64 (doubles) of a handle with M rows (Mpad padded) and N samples (Npad padded) at sketch width L: the partial Grams of the
// sample side, of B = A Q and of any factor of fewer rows, the column sums, the abs-max partials of a 32-column block, and the two
// partial arrays of the orthonormalisation's tail
inline int64_t part64_capacity(int64_t M, int64_t Mpad, int64_t N, int64_t Npad, int L) {
    return std::max({std::max(gram_num_parts(N), gram_max_parts(std::max(M, N))) * (int64_t)L * L, colsum_num_parts(Npad) * (int64_t)L,
                     absmax_num_parts(Mpad) * (int64_t)32, 2 * tail_num_parts(Npad) * (int64_t)L});
}
// d_cpart (floats): c partials per K1 wave x L (f32 path), per 64-row group x L (Omega, launch_scale_rows), or per 32-row unit x 32 per
// 32-column block (exact path)
inline int64_t cpart_capacity(int64_t gq_waves, int64_t Mpad, int L) {
    return std::max({gq_waves * (int64_t)L, omega_num_parts(Mpad) * (int64_t)L, Mpad * (int64_t)(L / 32)});
}
// d_cand_val / d_cand_idx (elements): one candidate per workgroup of launch_scores and column
inline int64_t scores_cand_capacity() { return (int64_t)kScoreParts * kMaxSketchCols; }
// the workspace of one gpca_project call (Lp = columns rounded up to 32): scratch of the sum of c (doubles), the abs-max partials of a
// 32-column block or the 2 * Lp gathered column maxima of a sharded model (doubles), the c partials of one side (floats)
inline int64_t project_scratch_capacity(int Lp) { return sum_scratch_need(Lp); }
inline int64_t project_part_capacity(int64_t Mpad, int Lp) { return std::max<int64_t>(absmax_num_parts(Mpad) * 32, 2 * (int64_t)Lp); }
inline int64_t project_cpart_capacity(int64_t Mpad, int Lp) { return omega_num_parts(Mpad) * (int64_t)Lp; }

// ---- windowed LD (ld.hip, gpca_ld.cpp) -------------------------------------------------------------------------------------------
// A workgroup owns kLdRows consecutive kept rows of the band (two 32-row tiles, first row i0) and one chunk of kLdCols columns (four
// 32-column tiles, one per wave) of the span that starts at i0; it walks the samples in stages of kLdStage.
constexpr int kLdRows = 64, kLdCols = 128, kLdStage = 128, kLdThreads = 256;
constexpr int kLdProducts = 6;                       // sum g'g', g'm, mg', g'^2 m, m g'^2, mm: i32 planes of the call's workspace
inline int64_t ld_row_blocks(int64_t rows) { return (rows + kLdRows - 1) / kLdRows; }
// 32-column tiles from i0 that a row block's widest window (weff slots) reaches: its last column is i0 + kLdRows - 1 + weff
inline int64_t ld_col_tiles(int64_t weff) { return (kLdRows - 1 + weff) / 32 + 1; }
inline int64_t ld_col_chunks(int64_t weff) { return (ld_col_tiles(weff) + kLdCols / 32 - 1) / (kLdCols / 32); }
inline int64_t ld_stages(int64_t N) { return (N + kLdStage - 1) / kLdStage; }
// stages per workgroup when the sample axis is split so that about 1 024 workgroups exist (the partial sums meet in i32 atomics)
inline int64_t ld_stages_per_split(int64_t nblocks, int64_t nst) {
    int64_t S = nblocks >= 1024 ? 1 : (1024 + nblocks - 1) / std::max<int64_t>(nblocks, 1);
    if (S > nst) S = nst;
    if (S < 1) S = 1;
    return (nst + S - 1) / S;
}
inline int64_t ld_splits(int64_t nblocks, int64_t nst) { const int64_t per = ld_stages_per_split(nblocks, nst); return (nst + per - 1) / per; }
constexpr int64_t ld_above_words(int64_t wmax) { return (wmax + 63) / 64; }
// elements of the call's buffers: the product planes (i32), one plane after the other; the per-row sums of rows [row0, hi) (u32:
// sum g', sum g'^2, missing); r2 / counts / above of the band
inline int64_t ld_ws_capacity(int64_t rows, int64_t wmax) { return (int64_t)kLdProducts * rows * wmax; }
inline int64_t ld_stat_capacity(int64_t row0, int64_t hi) { return 3 * (hi - row0); }
inline int64_t ld_r2_capacity(int64_t rows, int64_t wmax) { return rows * wmax; }
inline int64_t ld_counts_capacity(int64_t rows, int64_t wmax) { return 6 * rows * wmax; }
inline int64_t ld_above_capacity(int64_t rows, int64_t wmax) { return rows * ld_above_words(wmax); }

// ---- LD scores from the product planes of the banded sweep (k_ld_score in ld.hip, gpca_ld_score.cpp) -----------------------------
// A workgroup owns a tile of kLdScoreRows band rows x kLdScoreSlots slots of the planes.  Thread p owns the partner row
// t0 + d0 + 1 + p of the tile (an anti-diagonal: kLdScoreRows + kLdScoreSlots - 1 of them) and walks the tile's rows, so in every
// step the threads read consecutive slots of one row.
constexpr int kLdScoreRows = 64, kLdScoreSlots = 256;
constexpr int kLdScoreThreads = kLdScoreRows + kLdScoreSlots;              // 320 = 5 waves; the last thread owns no partner
constexpr int kLdScoreMaxWmax = 1 << 20;                                  // 2 wmax pairs of at most 2^41 each stay below 2^63
// a pair adds (1 << kLdScoreCountShift) + q, |q| <= 2^40, to a 64-bit sum of at most kLdScoreSlots pairs: count and sum in one word
constexpr int kLdScoreCountShift = 50;
inline int64_t ld_score_row_tiles(int64_t rows) { return (rows + kLdScoreRows - 1) / kLdScoreRows; }
inline int64_t ld_score_slot_tiles(int64_t weff) { return (weff + kLdScoreSlots - 1) / kLdScoreSlots; }
inline int64_t ld_score_grid(int64_t rows, int64_t weff) { return ld_score_row_tiles(rows) * ld_score_slot_tiles(weff); }
// rows that a band's sums reach, from row0: its own rows and the partners of its windows
inline int64_t ld_score_span(int64_t K, int64_t row0, int64_t row1, int64_t wmax) { return std::min(K, row1 + wmax) - row0; }
// elements of acc (i64) and partners (i32)
inline int64_t ld_score_acc_capacity(int64_t K, int64_t row0, int64_t row1, int64_t wmax) { return ld_score_span(K, row0, row1, wmax); }
inline int64_t ld_score_partners_capacity(int64_t K, int64_t row0, int64_t row1, int64_t wmax) { return ld_score_span(K, row0, row1, wmax); }

// ---- PC-Relate (pcrelate.hip, gpca_pcrelate.cpp) ---------------------------------------------------------------------------------
// A workgroup owns one kPcrTile x kPcrTile tile of the sample triangle (tile row >= tile column) and walks the kept rows in stages of
// kPcrStageRows; the f32 partial sums go to f64 running sums once per kPcrFlushRows kept rows, counted from the first kept row.
constexpr int kPcrTile = 128, kPcrThreads = 512, kPcrStageRows = 16, kPcrFlushRows = 256, kPcrMaxPcs = 32;
constexpr int kPcrBetaRows = 64;                     // kept rows per workgroup of the regression kernel (one lane per row)
constexpr int kPcrBetaWaves = 4;                     // its waves split the P + 1 coefficients between them
static_assert(kPcrFlushRows % kPcrStageRows == 0 && kPcrBetaRows % kPcrStageRows == 0 && kPcrStageRows % 8 == 0, "stage, flush group, beta block");
inline int64_t pcr_kpad(int64_t K) { return (K + kPcrBetaRows - 1) / kPcrBetaRows * kPcrBetaRows; }
inline int64_t pcr_npad(int64_t N) { return (N + kPcrTile - 1) / kPcrTile * kPcrTile; }
constexpr int64_t pcr_stages(int64_t K) { return (K + kPcrStageRows - 1) / kPcrStageRows; }
// coefficients of the hat matrix one wave of the regression kernel carries: P + 1 of them spread over kPcrBetaWaves waves, rounded up
// to a width the kernel is instantiated for
inline int pcr_beta_width(int P) {
    const int w = (P + 1 + kPcrBetaWaves - 1) / kPcrBetaWaves;
    for (int c : {1, 2, 3, 4, 6, 9}) if (w <= c) return c;
    return 0;
}
// elements of the call's buffers: beta in groups of 8 rows [kpad / 8][P + 1][8] (f32) and row-major [K][P + 1]; the design rows
// [npad][P + 1] (f32, zero past N); the hat matrix per wave of the regression kernel [waves][N][width] (f64); the invalid counts [npad]
inline int64_t pcr_beta_capacity(int64_t K, int P) { return pcr_kpad(K) * (int64_t)(P + 1); }
inline int64_t pcr_x_capacity(int64_t N, int P) { return pcr_npad(N) * (int64_t)(P + 1); }
inline int64_t pcr_hat_capacity(int64_t N, int P) { return (int64_t)kPcrBetaWaves * N * pcr_beta_width(P); }
inline int64_t pcr_inv_capacity(int64_t N) { return pcr_npad(N); }

// ---- bands of the sample triangle (gpca_grm, gpca_king, gpca_pcrelate: the kernels, their finish passes and the host front end) ----
// A call computes the rows [row0, row1) of the lower triangle of the N x N sample matrix, packed row-major; diag: the diagonal belongs
// to it (GRM, PC-Relate) or not (KING).  A workgroup owns one tile x tile block (tile row >= tile column) that meets the band.
constexpr int kGrmTile = 64, kKingTile = 128;        // samples per side of a workgroup's tile (PC-Relate: kPcrTile)
constexpr int64_t band_entries(int64_t row0, int64_t row1, bool diag) {
    return diag ? row1 * (row1 + 1) / 2 - row0 * (row0 + 1) / 2 : row1 * (row1 - 1) / 2 - row0 * (row0 - 1) / 2;
}
// entry (a, b) of the band, row0 <= a, b <= a (diag) or b < a
constexpr int64_t band_index(int64_t row0, int64_t a, int64_t b, bool diag) {
    return (diag ? a * (a + 1) / 2 - row0 * (row0 + 1) / 2 : a * (a - 1) / 2 - row0 * (row0 - 1) / 2) + b;
}
constexpr int64_t band_tile_count(int64_t row0, int64_t row1, int tile) {
    return ((row1 + tile - 1) / tile) * ((row1 + tile - 1) / tile + 1) / 2 - (row0 / tile) * (row0 / tile + 1) / 2;
}
// the band's tiles (x = tile row, y = tile column <= x) in the order the workgroups take them; Tile: int2 or anything like it
template <class Tile>
inline void band_tile_list(int64_t row0, int64_t row1, int tile, std::vector<Tile>& tiles) {
    tiles.clear();
    tiles.reserve((size_t)band_tile_count(row0, row1, tile));
    for (int64_t ta = row0 / tile; ta < (row1 + tile - 1) / tile; ++ta)
        for (int64_t tb = 0; tb <= ta; ++tb) { Tile t{}; t.x = (int)ta; t.y = (int)tb; tiles.push_back(t); }
}

// ---- linear association scan (assoc.hip, gpca_assoc.cpp) --------------------------------------------------------------------------
// A workgroup owns kAscRows consecutive kept rows of the band (32 per wave) and all L = T + Pc columns, padded to 32 or 64; it walks
// the samples in stages of kAscStage; the f32 partial sums go to f64 running sums once per kAscFlush samples, counted from sample 0.
constexpr int kAscRows = 128, kAscThreads = 256, kAscStage = 64, kAscFlush = 256, kAscMaxCols = 64;
constexpr int kAscGPitch = kAscStage + 8;            // bytes per row of a staged block of calls (ds_read_b64 stays 8-byte aligned)
constexpr int kAscBPitch = kAscStage + 4;            // floats per column of a staged panel of B (ds_read_b128 stays 16-byte aligned)
static_assert(kAscFlush % kAscStage == 0 && kAscStage % 32 == 0 && kAscThreads * 32 == kAscRows * kAscStage, "stage, flush group, staging map");
constexpr int asc_lpad(int L) { return L <= 32 ? 32 : 64; }
constexpr int64_t asc_npad(int64_t N) { return (N + kAscStage - 1) / kAscStage * kAscStage; }
constexpr int64_t asc_stages(int64_t N) { return (N + kAscStage - 1) / kAscStage; }
constexpr int64_t asc_row_blocks(int64_t rows) { return (rows + kAscRows - 1) / kAscRows; }
// elements of the call's buffers: B^T [asc_lpad(L)][asc_npad(N)] (f32, zero past N and past L); the include mask, one bit per sample
// (u32 words, zero past N); xb [rows][L] (f64); the per-row sums [rows][3] (u32: n_obs, sum g', sum g'^2); stats [rows][T][3] and
// rowinfo [rows][4] (f64)
constexpr int64_t asc_b_capacity(int64_t N, int L) { return (int64_t)asc_lpad(L) * asc_npad(N); }
constexpr int64_t asc_inc_capacity(int64_t N) { return asc_npad(N) / 32; }
constexpr int64_t asc_xb_capacity(int64_t rows, int L) { return rows * (int64_t)L; }
constexpr int64_t asc_sums_capacity(int64_t rows) { return 3 * rows; }
constexpr int64_t asc_stats_capacity(int64_t rows, int T) { return 3 * rows * (int64_t)T; }
constexpr int64_t asc_info_capacity(int64_t rows) { return 4 * rows; }

// ---- logistic score scan (assoc_score.hip, gpca_assoc_score.cpp) ------------------------------------------------------------------
// The tile, the stages and the flush groups are k_assoc's (kAsc*, asc_npad, asc_stages, asc_row_blocks, asc_lpad, asc_b_capacity,
// asc_inc_capacity).  The panel holds Pc + 3 columns per trait, L = T (Pc + 3) <= kAsrMaxCols: the T columns w_t first (the product
// with the squared operand needs no other, and T <= 21 keeps them in the first block of 32), then the T columns r_t, then
// A_t,0 .. A_t,Pc trait by trait.  k_assoc_score_count: a wave counts one row, a lane 32 samples of each chunk of kAsrChunk.
constexpr int kAsrMaxCols = 64, kAsrCountRows = 4, kAsrCountThreads = 64 * kAsrCountRows, kAsrChunk = 64 * 32;
static_assert(kAsrMaxCols == kAscMaxCols && kAsrChunk % kAscStage == 0, "the score scan stages its panel as k_assoc does");
constexpr int asr_cols(int T, int Pc) { return T * (Pc + 3); }
constexpr int asr_max_traits(int Pc) { return kAsrMaxCols / (Pc + 3); }
constexpr int asr_col_w(int t) { return t; }
constexpr int asr_col_r(int T, int t) { return T + t; }
constexpr int asr_col_a(int T, int Pc, int t, int j) { return 2 * T + t * (Pc + 1) + j; }
constexpr int64_t asr_count_blocks(int64_t rows) { return (rows + kAsrCountRows - 1) / kAsrCountRows; }
constexpr int64_t asr_count_chunks(int64_t N) { return (asc_npad(N) + kAsrChunk - 1) / kAsrChunk; }
// elements of the call's own buffers: dv [rows][L] (f64, the panel's column order, gwg_t in the place of w_t); the per-row sums
// [rows][3] (u32); stats [rows][T][5], ua [rows][T][Pc + 3] and rowinfo [rows][5] (f64)
constexpr int64_t asr_dv_capacity(int64_t rows, int L) { return rows * (int64_t)L; }
constexpr int64_t asr_sums_capacity(int64_t rows) { return 3 * rows; }
constexpr int64_t asr_stats_capacity(int64_t rows, int T) { return 5 * rows * (int64_t)T; }
constexpr int64_t asr_ua_capacity(int64_t rows, int T, int Pc) { return rows * (int64_t)asr_cols(T, Pc); }
constexpr int64_t asr_info_capacity(int64_t rows) { return 5 * rows; }

// ---- saddle-point correction of the score scan (assoc_spa.hip, gpca_assoc_score.cpp) ----------------------------------------------
// The items (row, trait) of the band are flagged in ranges of kAspListItems; a range's flagged items are taken in turn by asp_slots(N)
// persistent workgroups of kAspThreads threads.  A workgroup stages a row in chunks of kAspChunk samples (a thread fetches 32, as in
// k_assoc_score_count) and keeps the item's g~ in its own slice of asp_gpad(N) doubles; a thread then owns the samples tid + kAspThreads k.
// The slices together hold at most kAspWsBytes, or one slice where a single one is larger: no extent but out grows with the band.
constexpr int kAspThreads = 256, kAspChunk = kAspThreads * 32, kAspMaxSlots = 1024;
constexpr int64_t kAspWsBytes = (int64_t)256 << 20, kAspListItems = (int64_t)1 << 20;
static_assert(kAspChunk % kAscStage == 0, "a chunk is whole stages: a fetch below asc_npad(N) stays inside the row's pitch");
constexpr int64_t asp_gpad(int64_t N) { return asc_npad(N); }
constexpr int64_t asp_chunks(int64_t N) { return (asp_gpad(N) + kAspChunk - 1) / kAspChunk; }
constexpr int64_t asp_slots(int64_t N) {
    const int64_t s = kAspWsBytes / (8 * asp_gpad(N > 0 ? N : 1));
    return s < 1 ? 1 : (s > kAspMaxSlots ? kAspMaxSlots : s);
}
// the workgroups a correction launches: asp_slots(N), or what GPCA_ASP_SLOTS forces (want > 0), clamped to [1, asp_slots(N)]; the
// workspace keeps asp_slots(N) slices, so a forced count only leaves slices unused
constexpr int64_t asp_clamp_slots(int64_t N, int64_t want) {
    const int64_t s = asp_slots(N);
    return want <= 0 || want > s ? s : want;
}
constexpr int64_t asp_ranges(int64_t rows, int T) { return (rows * (int64_t)T + kAspListItems - 1) / kAspListItems; }
// elements of the call's own buffers: g~ [asp_slots][asp_gpad] (f64); Z [T][Pc + 1][asp_gpad] and mu [T][asp_gpad] (f64, 0 outside S and
// past N); the list of a range's flagged items (i32, relative to the range) and out [rows][T][4] (f64)
constexpr int64_t asp_g_capacity(int64_t N) { return asp_slots(N) * asp_gpad(N); }
constexpr int64_t asp_z_capacity(int64_t N, int T, int Pc) { return (int64_t)T * (Pc + 1) * asp_gpad(N); }
constexpr int64_t asp_mu_capacity(int64_t N, int T) { return (int64_t)T * asp_gpad(N); }
constexpr int64_t asp_list_capacity(int64_t rows, int T) { return rows * (int64_t)T < kAspListItems ? rows * (int64_t)T : kAspListItems; }
constexpr int64_t asp_out_capacity(int64_t rows, int T) { return 4 * rows * (int64_t)T; }

// ---- Firth correction of the score scan (assoc_firth.hip, gpca_assoc_score.cpp) ----------------------------------------------------
// The item ranges, the persistent workgroups, the chunks and the buffers g~, Z, mu and list are the saddle-point correction's (asp_*
// above); only the result differs: out [rows][T][kAfiWidth] (f64) = -log10 p, status, beta, se, the likelihood-ratio statistic
constexpr int kAfiWidth = 5;
constexpr int64_t afi_out_capacity(int64_t rows, int T) { return (int64_t)kAfiWidth * rows * (int64_t)T; }

// The device bytes a logistic scan allocates for a band of `rows` kept rows (gpca_assoc_score.cpp: the sum its GPCA_ERR_OOM check takes
// before any allocation, without that check's slack).  dstats / ua / info: the buffer exists; corr_out: the elements of a
// correction's result (asp_out_capacity or afi_out_capacity; 0 without a correction); correct: some item may be corrected (the
// cutoff is finite), so Z, mu and the slices of g~ exist.
constexpr double asr_call_bytes(int64_t N, int64_t rows, int T, int Pc, bool dstats, bool ua, bool info, int64_t corr_out, bool correct) {
    const int L = asr_cols(T, Pc);
    double b = 4.0 * (double)asc_b_capacity(N, L) + 4.0 * (double)asc_inc_capacity(N) + 8.0 /* the invalid-genotype word */ +
               8.0 * (double)asr_dv_capacity(rows, L) + 4.0 * (double)asr_sums_capacity(rows);
    if (dstats) b += 8.0 * (double)asr_stats_capacity(rows, T);
    if (ua) b += 8.0 * (double)asr_ua_capacity(rows, T, Pc);
    if (info) b += 8.0 * (double)asr_info_capacity(rows);
    if (corr_out > 0) b += 8.0 * (double)corr_out + 4.0 * (double)asp_list_capacity(rows, T) + 4.0 /* the list's counter */;
    if (correct) b += 8.0 * (double)(asp_g_capacity(N) + asp_z_capacity(N, T, Pc) + asp_mu_capacity(N, T));
    return b;
}

// ---- gene-level set tests of the score scan (assoc_set.hip, gpca_assoc_score.cpp) ---------------------------------------------------
// A set lists 1 <= m <= kAsgMaxRows rows; its Phi is stored per trait as the packed lower triangle, row by row: entry (a, b), b <= a,
// at asg_tri(a) + b of asg_tri(m).  The lower triangle is cut into strips of kAsgStripRows rows; a workgroup of kAsgThreads threads owns
// one (strip, trait): it stages the set's rows [0, asg_staged_rows(m, s)) with the score scan's staging map (thread t: half t & 1 of row
// t / 2, stages of kAscStage samples, flush every kAscFlush), and wave v <= s owns the 32 x 32 tile (strip s, column block v).
constexpr int kAsgMaxRows = 128, kAsgStripRows = 32, kAsgThreads = 256;
static_assert(kAsgMaxRows == kAscRows && kAsgThreads == kAscThreads && kAsgMaxRows == kMaxSketchCols, "a set is one score-scan tile and one host eigenproblem");
static_assert(kAsgMaxRows / kAsgStripRows == kAsgThreads / 64, "a wave per column block of the last strip");
constexpr int64_t asg_tri(int64_t m) { return m * (m + 1) / 2; }
constexpr int asg_strips(int m) { return (m + kAsgStripRows - 1) / kAsgStripRows; }
constexpr int asg_staged_rows(int m, int s) { return kAsgStripRows * (s + 1) < m ? kAsgStripRows * (s + 1) : m; }
// one strip of the call: its set's first listed row, the set's first Phi element (of trait 0), the set's size and the strip's index
struct AsgStrip { int64_t l0, p0; int32_t m, s; };
// where Phi_ab (b <= a) of trait t lies: p0 = T times the packed entries of the sets before this one
constexpr int64_t asg_phi_index(int64_t p0, int m, int t, int a, int b) { return p0 + (int64_t)t * asg_tri(m) + asg_tri(a) + b; }
// elements of the Gram's buffers: the listed rows' original rows (i64), the strips (AsgStrip), Phi (f64)
constexpr int64_t asg_rows_capacity(int64_t listed) { return listed; }
constexpr int64_t asg_strip_capacity(int64_t strips) { return strips; }
constexpr int64_t asg_phi_capacity(int64_t tri_total, int T) { return tri_total * (int64_t)T; }
// The device bytes a set call allocates (gpca_assoc_logistic_set's GPCA_ERR_OOM sum, without the check's slack): the score scan's for the
// listed rows, plus the three buffers above.
constexpr double asg_call_bytes(int64_t N, int64_t listed, int64_t strips, int64_t tri_total, int T, int Pc, bool dstats, bool ua, bool info) {
    return asr_call_bytes(N, listed, T, Pc, dstats, ua, info, 0, false) + 8.0 * (double)asg_rows_capacity(listed) +
           (double)sizeof(AsgStrip) * (double)asg_strip_capacity(strips) + 8.0 * (double)asg_phi_capacity(tri_total, T);
}

// ---- per-group genotype counts (group_counts.hip, gpca_group_counts.cpp) -----------------------------------------------------------
// A workgroup of kGcThreads threads owns kGcRows consecutive kept rows of the band (32 per wave) and all P <= kGcMaxGroups groups,
// padded to 32 or 64 one-hot columns; it walks the samples in stages of kGcStage with the scans' staging map (thread t: the 32 samples
// of half t & 1 of row t / 2) and multiplies blocks of kGcBlock samples (one v_mfma_i32_32x32x32_i8 per plane and column block; the
// missing plane only where a wave ballot over its 32 rows x kGcBlock samples finds a missing call).  No split of the sample axis: a
// workgroup writes the counts of its rows once.
constexpr int kGcRows = 128, kGcThreads = 256, kGcStage = 64, kGcBlock = 32, kGcMaxGroups = 64;
constexpr int kGcPitch = kGcStage + 16;              // bytes per staged row of calls and per staged one-hot column (ds_read_b128 stays 16-byte aligned)
static_assert(kGcStage == kAscStage && kGcThreads * 32 == kGcRows * kGcStage && kGcStage % kGcBlock == 0, "the scans' stage and staging map");
static_assert(kGcMaxGroups * (kGcStage / 16) == kGcThreads, "a thread stages 16 bytes of one one-hot column");
constexpr int gc_ppad(int P) { return P <= 32 ? 32 : 64; }
constexpr int64_t gc_npad(int64_t N) { return asc_npad(N); }
constexpr int64_t gc_stages(int64_t N) { return asc_stages(N); }
constexpr int64_t gc_row_blocks(int64_t rows) { return (rows + kGcRows - 1) / kGcRows; }
// where thread t of a stage reads its 16 one-hot bytes of stage s (column t / 4, quarter t & 3), and where a workgroup's thread t
// reads its 32 samples of a row (a byte offset into the row: int8 32 bytes, 2-bit 8 bytes)
constexpr int64_t gc_onehot_offset(int64_t npad, int t, int64_t s) { return (int64_t)(t >> 2) * npad + s * kGcStage + 16 * (t & 3); }
constexpr int64_t gc_row_offset(bool packed, int t, int64_t s) { return packed ? (s * kGcStage + 32 * (t & 1)) >> 2 : s * kGcStage + 32 * (t & 1); }
// where the count c (0 n_obs, 1 n_het, 2 n_hom2) of band row r and group p lies
constexpr int64_t gc_counts_index(int64_t r, int P, int p, int c) { return (r * P + p) * 3 + c; }
// elements of the call's buffers: the one-hot matrix [gc_ppad(P)][gc_npad(N)] (bytes, zero past N, past P and on label -1); the labels
// [N] (i32); the group sizes [kGcMaxGroups] (u32); counts [rows][P][3] (u32); the invalid-genotype word (8 bytes)
constexpr int64_t gc_onehot_capacity(int64_t N, int P) { return (int64_t)gc_ppad(P) * gc_npad(N); }
constexpr int64_t gc_label_capacity(int64_t N) { return N; }
constexpr int64_t gc_size_capacity() { return kGcMaxGroups; }
constexpr int64_t gc_counts_capacity(int64_t rows, int P) { return 3 * rows * (int64_t)P; }
// The device bytes a call allocates (gpca_group_counts' GPCA_ERR_OOM sum, without the check's slack)
constexpr double gc_call_bytes(int64_t N, int64_t rows, int P) {
    return (double)gc_onehot_capacity(N, P) + 4.0 * (double)gc_label_capacity(N) + 4.0 * (double)gc_size_capacity() +
           4.0 * (double)gc_counts_capacity(rows, P) + 8.0;
}

// ---- f2 jackknife blocks from the counts workspace (f2_blocks.hip, gpca_f2_blocks.cpp) -----------------------------------------------
// A workgroup of kFbThreads threads owns kFbRun consecutive band rows, in LDS tiles of kFbTile rows.  Per tile, thread t forms p and
// h = (p (1 - p)) / (n - 1) of group t % kFbPitch of rows t / kFbPitch + (kFbThreads / kFbPitch) k (a wave per row: the row's validity
// mask is one ballot); then thread t owns the pairs t, t + kFbThreads, ... (at most kFbSlots), whose i64 sums and i32 counts stay in
// registers while the block id stays the same.
constexpr int kFbThreads = 256, kFbTile = 32, kFbRun = 256, kFbPitch = 64, kFbSlots = 8;
constexpr int64_t kFbMaxRows = (int64_t)1 << 21;     // rows of a call: |q| <= 1.5 x 2^40 < 2^41 per row, so a sum stays below 2^62
constexpr double kFbScale = 1099511627776.0;         // 2^40
static_assert(kFbPitch == kGcMaxGroups && kFbPitch == 64 && kFbThreads % kFbPitch == 0 && kFbRun % kFbTile == 0, "a wave stages one row's groups");
static_assert(kFbTile % (kFbThreads / kFbPitch) == 0, "the staging loop covers a tile in whole passes");
static_assert(kFbSlots * kFbThreads >= kGcMaxGroups * (kGcMaxGroups - 1) / 2, "every pair has a register slot");
constexpr int fb_pairs(int P) { return P * (P - 1) / 2; }
constexpr int fb_slots(int P) { return (fb_pairs(P) + kFbThreads - 1) / kFbThreads; }
// the pair map: pair q = i (i - 1) / 2 + j with j < i; fb_pair_i walks i up from 1 (at most kGcMaxGroups steps, once per thread and slot)
constexpr int fb_pair_index(int i, int j) { return i * (i - 1) / 2 + j; }
constexpr int fb_pair_i(int q) { int i = 1; while ((i + 1) * i / 2 <= q) ++i; return i; }
constexpr int fb_pair_j(int q) { return q - fb_pair_i(q) * (fb_pair_i(q) - 1) / 2; }
constexpr int64_t fb_row_blocks(int64_t rows) { return (rows + kFbRun - 1) / kFbRun; }
// the staging map: pass k of thread t stages (tile row, group); the LDS index of a (tile row, group) value
constexpr int fb_stage_passes() { return kFbTile / (kFbThreads / kFbPitch); }
constexpr int fb_stage_row(int t, int k) { return t / kFbPitch + (kFbThreads / kFbPitch) * k; }
constexpr int fb_stage_group(int t) { return t % kFbPitch; }
constexpr int fb_lds_index(int r, int g) { return r * kFbPitch + g; }
constexpr int fb_lds_values() { return kFbTile * kFbPitch; }                  // doubles of each of the two LDS planes (p and h)
constexpr int fb_lds_bytes() { return 2 * 8 * fb_lds_values() + 8 * kFbTile + 4 * kFbTile; }   // + the masks (u64) and the block ids (i32)
// where the sum and the count of (block b, pair q) lie
constexpr int64_t fb_out_index(int64_t b, int P, int q) { return b * fb_pairs(P) + q; }
// elements of the call's own buffers: the block ids [rows] (i32), the sums [B][pairs] (i64), the counts [B][pairs] (i32)
constexpr int64_t fb_block_capacity(int64_t rows) { return rows; }
constexpr int64_t fb_out_capacity(int64_t B, int P) { return B * (int64_t)fb_pairs(P); }
// The device bytes a call allocates (gpca_f2_blocks' GPCA_ERR_OOM sum, without the check's slack): the group-counts pass and the above
constexpr double fb_call_bytes(int64_t N, int64_t rows, int P, int64_t B) {
    return gc_call_bytes(N, rows, P) + 4.0 * (double)fb_block_capacity(rows) + (8.0 + 4.0) * (double)fb_out_capacity(B, P);
}

// ---- per-sample genotype counts (sample_counts.hip, gpca_sample_counts.cpp) ---------------------------------------------------------
// A thread owns kScLane consecutive samples (one uint4 of an int8 row, one dword of a 2-bit row); a workgroup of kScThreads threads (one
// wave) owns a chunk of kScChunk samples and one of the plan's row splits: the band's kept rows [split * per, (split + 1) * per).  The
// workgroups are numbered split-major on a one-dimensional grid.  A thread counts missing, het and hom2 calls of its 16 samples in
// byte-wise counters that it adds to u32 registers once per kScFlushRows rows (< 256), fetching kScUnroll rows at a time; it writes its
// sums to the slab of its split, and a second kernel adds the slabs of a sample.
constexpr int kScThreads = 64, kScLane = 16, kScChunk = kScThreads * kScLane, kScUnroll = 8, kScFlushRows = 248, kScSumThreads = 256;
// the default split: about this many waves per CU (four rounds of the 2 resident waves per SIMD: one round leaves a tail wherever
// chunks x splits is not the slot count; 8 -> 32 took 2.68 -> 2.20 ms at 1M x 10k), and a split no shorter than kScMinRows rows
constexpr int kScWavesPerCu = 32, kScMinRows = 256;
static_assert(kScFlushRows % kScUnroll == 0 && kScFlushRows <= 255, "a byte counter holds a flush group; a flush group is whole fetch groups");
constexpr int64_t sc_npad(int64_t N) { return (N + kScLane - 1) / kScLane * kScLane; }
constexpr int64_t sc_chunks(int64_t N) { return (N + kScChunk - 1) / kScChunk; }
struct ScPlan { int64_t chunks, splits, per; };      // per = kept rows of a split (the last one may hold fewer)
// forced > 0 (GPCA_SAMPLE_COUNTS_SPLITS): that many splits, clamped to the band's rows
inline ScPlan sc_plan(int64_t rows, int64_t N, int cus, int64_t forced = 0) {
    ScPlan p{};
    p.chunks = sc_chunks(N > 0 ? N : 1);
    int64_t s = forced > 0 ? forced : ((int64_t)kScWavesPerCu * (cus > 0 ? cus : 1) + p.chunks - 1) / p.chunks;
    if (forced <= 0) s = std::min<int64_t>(s, (rows + kScMinRows - 1) / kScMinRows);
    s = std::max<int64_t>(1, std::min<int64_t>(s, std::max<int64_t>(rows, 1)));
    p.per = (std::max<int64_t>(rows, 1) + s - 1) / s;
    p.splits = (std::max<int64_t>(rows, 1) + p.per - 1) / p.per;
    return p;
}
constexpr int64_t sc_grid(const ScPlan& p) { return p.chunks * p.splits; }
// the sample a thread's 16 start at, and the byte offset of its fetch into a row (int8: 16 bytes, 2-bit: 4 bytes)
constexpr int64_t sc_thread_sample(int64_t chunk, int t) { return (chunk * kScThreads + t) * kScLane; }
constexpr int64_t sc_row_offset(bool packed, int64_t n0) { return packed ? n0 >> 2 : n0; }
// where a split's sums of sample n lie: part [splits][npad][3] (u32: missing, het, hom2), qpart [splits][npad] (u64: the q of the rows
// on which n is missing)
constexpr int64_t sc_part_index(int64_t split, int64_t npad, int64_t n, int c) { return (split * npad + n) * 3 + c; }
constexpr int64_t sc_qpart_index(int64_t split, int64_t npad, int64_t n) { return split * npad + n; }
// elements of the call's buffers: the two slabs; counts [N][3] (u32) and qsum [N] (u64); q [rows] (u32); the invalid-genotype word
constexpr int64_t sc_part_capacity(int64_t splits, int64_t N) { return 3 * splits * sc_npad(N); }
constexpr int64_t sc_qpart_capacity(int64_t splits, int64_t N) { return splits * sc_npad(N); }
constexpr int64_t sc_counts_capacity(int64_t N) { return 3 * N; }
constexpr int64_t sc_qsum_capacity(int64_t N) { return N; }
constexpr int64_t sc_q_capacity(int64_t rows) { return rows; }
// The device bytes a call allocates (gpca_sample_counts' GPCA_ERR_OOM sum, without the check's slack)
constexpr double sc_call_bytes(int64_t N, int64_t rows, int64_t splits, bool hasq) {
    return 4.0 * (double)sc_part_capacity(splits, N) + 4.0 * (double)sc_counts_capacity(N) + 8.0 +
           (hasq ? 8.0 * (double)sc_qpart_capacity(splits, N) + 8.0 * (double)sc_qsum_capacity(N) + 4.0 * (double)sc_q_capacity(rows) : 0.0);
}

// ---- runs of homozygosity (roh.hip, gpca_roh.cpp) ----------------------------------------------------------------------------------
// The access pattern and the launch plan are the sample counts': a thread owns kScLane consecutive samples, a workgroup (one wave) a
// chunk of kScChunk samples and one row split [split * per, (split + 1) * per) of the band.  Rows are band-relative (0 .. rows - 1)
// everywhere below.  k_roh_mark decides the rows of its split: inside every window domain [d0, d1) that the split meets it walks the
// windows [roh_win_lo, roh_win_hi] (window s = rows s .. s + W - 1), so it reads rows roh_win_lo .. roh_win_hi + W - 1: its own rows and
// a halo of at most W - 1 rows on either side, clipped at the domain.  It writes one bit per (row, sample) to the plane.  k_roh_runs
// walks the plane over its split's rows and leaves what crosses a split boundary in rec; k_roh_stitch joins it, a thread per sample.
constexpr int kRohMaxWindow = 64, kRohUnroll = 4, kRohFlushRows = 255, kRohStitchThreads = 64, kRohStitchBatch = 8;
constexpr int kRohMaxDen = 1 << 20;
using RohPlan = ScPlan;
// forced > 0 (GPCA_ROH_SPLITS): that many splits, clamped to the band's rows
inline RohPlan roh_plan(int64_t rows, int64_t N, int cus, int64_t forced = 0) { return sc_plan(rows, N, cus, forced); }
constexpr int64_t roh_npad(int64_t N) { return sc_npad(N); }
// the windows a piece [pa, pb) of the domain [d0, d1) needs (d1 - d0 >= W): first and last window start
constexpr int64_t roh_win_lo(int64_t d0, int64_t pa, int W) { return pa - W + 1 > d0 ? pa - W + 1 : d0; }
constexpr int64_t roh_win_hi(int64_t d1, int64_t pb, int W) { return pb - 1 < d1 - W ? pb - 1 : d1 - W; }
// the windows that cover row j of the domain: roh_cov_lo .. roh_cov_hi (cov = hi - lo + 1, 1 .. W)
constexpr int64_t roh_cov_lo(int64_t d0, int64_t j, int W) { return j - W + 1 > d0 ? j - W + 1 : d0; }
constexpr int64_t roh_cov_hi(int64_t d1, int64_t j, int W) { return j < d1 - W ? j : d1 - W; }
// the plane: inroh [rows][pitch] bytes, bit (n & 7) of byte n / 8 of a row = sample n; a thread writes the two bytes of its 16 samples
constexpr int64_t roh_plane_pitch(int64_t N) { return roh_npad(N) / 8; }
constexpr int64_t roh_plane_index(int64_t j, int64_t pitch, int64_t n0) { return j * pitch + (n0 >> 3); }
constexpr int64_t roh_plane_capacity(int64_t rows, int64_t N) { return rows * roh_plane_pitch(N); }
// cnt [splits][npad] u32: the reported runs that start in the split, then (k_roh_stitch, in place) the runs of the sample in the splits
// before it
constexpr int64_t roh_cnt_index(int64_t split, int64_t npad, int64_t n) { return split * npad + n; }
constexpr int64_t roh_cnt_capacity(int64_t splits, int64_t N) { return splits * roh_npad(N); }
// rec [splits][npad][kRohRecWords] u32, what a split knows of a sample: the head = the continuation of a run of the split before (its
// rows in this split, their het and missing calls; flag kRohFlagThrough: it goes on into the next split), the tail = a run that starts in
// the split and goes on into the next one (flag kRohFlagTail; its first row, its het and missing calls in this split), and the split's
// own reported runs.  Words: head rows, head het, head missing, flags, tail first, tail het, tail missing, own runs
constexpr int kRohRecWords = 8;
constexpr unsigned kRohFlagThrough = 1u, kRohFlagTail = 2u;
constexpr int64_t roh_rec_index(int64_t split, int64_t npad, int64_t n) { return (split * npad + n) * kRohRecWords; }
constexpr int64_t roh_rec_capacity(int64_t splits, int64_t N) { return splits * roh_npad(N) * kRohRecWords; }
// elements of the call's other buffers: brk [rows] u8; dom [domains + 1] i32 (the domains' first rows, then rows); seg_count [N] u32;
// base [N] u64 (the records of the samples before n); segs [records][5] u32; the invalid-genotype word
constexpr int64_t roh_brk_capacity(int64_t rows) { return rows; }
constexpr int64_t roh_dom_capacity(int64_t domains) { return domains + 1; }
constexpr int64_t roh_segcount_capacity(int64_t N) { return N; }
constexpr int64_t roh_base_capacity(int64_t N) { return N; }
constexpr int64_t roh_seg_capacity(int64_t records) { return 5 * records; }
// The device bytes a call allocates (gpca_roh's GPCA_ERR_OOM sum, without the check's slack); records = min(cap, n_found)
constexpr double roh_call_bytes(int64_t N, int64_t rows, int64_t splits, int64_t domains, int64_t records) {
    return (double)roh_plane_capacity(rows, N) + (double)roh_brk_capacity(rows) + 4.0 * (double)roh_dom_capacity(domains) +
           4.0 * (double)roh_cnt_capacity(splits, N) + 4.0 * (double)roh_rec_capacity(splits, N) + 4.0 * (double)roh_segcount_capacity(N) + 8.0 * (double)roh_base_capacity(N) +
           4.0 * (double)roh_seg_capacity(records) + 8.0;
}

// ---- admixture proportions: one EM step and the fit around it (admix.hip, gpca_admix.cpp; include/gpca.h section a21) -----------------
// A workgroup of kAdmThreads threads owns a chunk of kAdmChunk samples (a thread per sample) and a block of kAdmRowBlock kept rows, which
// it walks in tiles of kAdmTile rows: a thread forms a and b of its sample on the tile's rows (the sums over rows stay in its registers)
// and leaves them in LDS, where the same threads, now as kAdmTile rows x kAdmGroups groups of kAdmGroupSamples samples, form the sums over
// the chunk's samples.  The plan is a function of (rows, N) alone: no CU count, no environment, no storage mode enters, so neither does
// any enter the order of a sum.  The workgroups are numbered block-major on a one-dimensional grid.
constexpr int kAdmMaxK = 16, kAdmThreads = 256, kAdmChunk = kAdmThreads, kAdmTile = 16, kAdmRowBlock = 4096;
constexpr int kAdmGroups = kAdmThreads / kAdmTile, kAdmGroupSamples = kAdmChunk / kAdmGroups, kAdmPitch = kAdmChunk + 1;
constexpr int kAdmSumThreads = 256, kAdmNormBlock = 4096;
static_assert(kAdmRowBlock % kAdmTile == 0 && kAdmGroups * kAdmGroupSamples == kAdmChunk && kAdmNormBlock % kAdmSumThreads == 0, "whole tiles, whole groups");
// the a and b tiles [2][kAdmTile][kAdmPitch] are reused for the groups' partial sums [kAdmMaxK][2][kAdmGroups][kAdmTile]
static_assert(2 * kAdmTile * kAdmPitch >= kAdmMaxK * 2 * kAdmGroups * kAdmTile, "the partial sums fit in the a and b tiles");
// the register width a kernel is compiled for: the columns K .. adm_kpad(K) - 1 are zeros, which add nothing to any sum
constexpr int adm_kpad(int K) { return K <= 4 ? 4 : K <= 8 ? 8 : 16; }
struct AdmPlan { int64_t chunks, blocks; };
constexpr AdmPlan adm_plan(int64_t rows, int64_t N) {
    return AdmPlan{((N > 0 ? N : 1) + kAdmChunk - 1) / kAdmChunk, ((rows > 0 ? rows : 1) + kAdmRowBlock - 1) / kAdmRowBlock};
}
constexpr int64_t adm_grid(const AdmPlan& p) { return p.chunks * p.blocks; }
// the slabs: fpart [chunks][rows][2][K] = the chunk's sums of a q and b q; qpart [blocks][N][K] = the block's sum of a f + b (1 - f);
// llpart [blocks][chunks] (f64) = the workgroup's log-likelihood terms
constexpr int64_t adm_fpart_index(int64_t chunk, int64_t rows, int64_t row, int ab, int K, int k) { return ((chunk * rows + row) * 2 + ab) * K + k; }
constexpr int64_t adm_qpart_index(int64_t block, int64_t N, int64_t n, int K, int k) { return (block * N + n) * K + k; }
constexpr int64_t adm_llpart_index(int64_t block, int64_t chunks, int64_t chunk) { return block * chunks + chunk; }
constexpr int64_t adm_fpart_capacity(const AdmPlan& p, int64_t rows, int K) { return p.chunks * rows * 2 * K; }
constexpr int64_t adm_qpart_capacity(const AdmPlan& p, int64_t N, int K) { return p.blocks * N * K; }
constexpr int64_t adm_llpart_capacity(const AdmPlan& p) { return p.blocks * p.chunks; }
constexpr int64_t adm_q_capacity(int64_t N, int K) { return N * K; }
constexpr int64_t adm_f_capacity(int64_t rows, int K) { return rows * K; }
// the norms of a SQUAREM cycle: blocks of kAdmNormBlock elements of (Q, then F), two f64 per block
constexpr int64_t adm_norm_blocks(int64_t N, int64_t rows, int K) { return (adm_q_capacity(N, K) + adm_f_capacity(rows, K) + kAdmNormBlock - 1) / kAdmNormBlock; }
constexpr int64_t adm_npart_capacity(int64_t N, int64_t rows, int K) { return 2 * adm_norm_blocks(N, rows, K); }
// The device bytes a call allocates (the GPCA_ERR_OOM sum, without the check's slack): `sets` parameter sets (Q, F) -- 2 for a step, 5
// for a fit --, the mode bytes, the three slabs, the norms' partials (a fit), the sums (3 f64) and the invalid-genotype word
constexpr double adm_call_bytes(int64_t N, int64_t rows, int K, int sets, bool fit) {
    const AdmPlan p = adm_plan(rows, N);
    return 4.0 * (double)sets * (double)(adm_q_capacity(N, K) + adm_f_capacity(rows, K)) + (double)N + 4.0 * (double)adm_fpart_capacity(p, rows, K) +
           4.0 * (double)adm_qpart_capacity(p, N, K) + 8.0 * (double)adm_llpart_capacity(p) +
           (fit ? 8.0 * (double)adm_npart_capacity(N, rows, K) : 0.0) + 24.0 + 8.0;
}
// The hold-out step (gpca.h section a22): the fold of the call (kept row i, sample j) is word i & 3 of the philox call of the quad i >> 2,
// so a tile of kAdmTile rows takes kAdmTile / 4 calls; tiles start at multiples of kAdmTile, so a quad never straddles two tiles.
constexpr int kAdmCvMinFolds = 2, kAdmCvMaxFolds = 64, kAdmCvQuad = 4;
static_assert(kAdmTile % kAdmCvQuad == 0 && kAdmRowBlock % kAdmCvQuad == 0, "whole quads in a tile");
constexpr uint32_t adm_cv_fold_of(uint32_t word, uint32_t folds) { return (uint32_t)(((uint64_t)word * folds) >> 32); }
// llpart of a hold-out step is [partial][2]: the training and the held-out log-likelihood terms of the (block, chunk)
constexpr int64_t adm_cv_llpart_index(int64_t block, int64_t chunks, int64_t chunk, int comp) { return adm_llpart_index(block, chunks, chunk) * 2 + comp; }
constexpr int64_t adm_cv_llpart_capacity(const AdmPlan& p) { return 2 * adm_llpart_capacity(p); }
// the sums of a hold-out step (2 f64: loglik, held_loglik) and its counts (2 u64: n_held, n_het_held; integer atomicAdd, one per workgroup)
constexpr int64_t adm_cv_sums_capacity() { return 2; }
constexpr int64_t adm_cv_count_capacity() { return 2; }
// The device bytes of a call that takes hold-out steps: adm_call_bytes with llpart at its [partial][2] size, the two sums and the counts
constexpr double adm_cv_call_bytes(int64_t N, int64_t rows, int K, int sets, bool fit) {
    const AdmPlan p = adm_plan(rows, N);
    return adm_call_bytes(N, rows, K, sets, fit) - 8.0 * (double)adm_llpart_capacity(p) + 8.0 * (double)adm_cv_llpart_capacity(p) +
           8.0 * (double)adm_cv_sums_capacity() + 8.0 * (double)adm_cv_count_capacity();
}

// ---- many-trait QTL scan (assoc_qtl.hip, gpca_assoc_qtl.cpp; include/gpca.h section a24) ----------------------------------------------
// The tile, the stages and the flush groups are k_assoc's.  A workgroup owns kAscRows kept rows x a strip of tw trait columns, which it
// walks in tiles of kQtlTile = kAscMaxCols columns, the whole sample loop per tile.  The trait panel is B^T [qtl_tpad(T)][asc_npad(N)]: a
// tile's panel is asc_b_capacity(N, kQtlTile) floats at qtl_tile_offset, so what a tile stages is what k_assoc stages of a 64-column call.
// A band goes in chunks of qtl_chunk_blocks(T) row blocks, so that the per-workgroup bests [row blocks][T] stay within kQtlBestBytes.
constexpr int kQtlTile = kAscMaxCols, kQtlMinTw = kQtlTile, kQtlMaxTw = 1024, kQtlMaxPc = 63, kQtlReduceThreads = 256;
constexpr int64_t kQtlMaxTraits = (int64_t)1 << 20, kQtlBestBytes = (int64_t)256 << 20, kQtlTargetGroups = 512;
constexpr int64_t qtl_tpad(int64_t T) { return (T + kQtlTile - 1) / kQtlTile * kQtlTile; }
constexpr int64_t qtl_tiles(int64_t T) { return qtl_tpad(T) / kQtlTile; }
constexpr int64_t qtl_tile_offset(int64_t tile, int64_t N) { return tile * kQtlTile * asc_npad(N); }
// a legal strip width: a power of two between kQtlMinTw and kQtlMaxTw (what GPCA_QTL_TW is clamped to: the largest one not above it)
constexpr int qtl_clamp_tw(int64_t tw) {
    int w = kQtlMinTw;
    while (w < kQtlMaxTw && 2 * (int64_t)w <= tw) w *= 2;
    return w;
}
constexpr int64_t qtl_strips(int64_t T, int tw) { return (qtl_tpad(T) + tw - 1) / tw; }
// the widest strip that still leaves kQtlTargetGroups workgroups (two per CU) to a launch of `blocks` row blocks; forced > 0: that width
constexpr int qtl_strip_width(int64_t blocks, int64_t T, int64_t forced = 0) {
    if (forced > 0) return qtl_clamp_tw(forced);
    int w = kQtlMaxTw;
    while (w > kQtlMinTw && blocks * qtl_strips(T, w) < kQtlTargetGroups) w /= 2;
    return w;
}
// the row blocks of one launch: the bests of a launch are [blocks][T] x 16 B (r2 f64, row i64)
constexpr int64_t qtl_chunk_blocks(int64_t T) { return kQtlBestBytes / (16 * T) > 1 ? kQtlBestBytes / (16 * T) : 1; }
static_assert(qtl_chunk_blocks(kQtlMaxTraits) * 16 * kQtlMaxTraits <= kQtlBestBytes && qtl_strips(kQtlMaxTraits, kQtlMinTw) <= 65535, "bests and grid.y at the widest call");
// elements of the call's buffers: the trait panel (f32), yy padded to whole tiles (f64, 1 past T), the covariate panel of the per-row
// pass (Pc = 0: one column of zeros), its xb, the per-row sums and rowinfo (asc_sums_capacity, asc_info_capacity), hit_count [rows] u32,
// the records (index [cap][2] u32, value [cap][2] f64), the bests of a launch and the running bests [T] (r2 f64, row i64)
constexpr int64_t qtl_b_capacity(int64_t N, int64_t T) { return qtl_tpad(T) * asc_npad(N); }
constexpr int64_t qtl_yy_capacity(int64_t T) { return qtl_tpad(T); }
constexpr int qtl_cov_cols(int Pc) { return Pc > 0 ? Pc : 1; }
constexpr int64_t qtl_q_capacity(int64_t N, int Pc) { return asc_b_capacity(N, qtl_cov_cols(Pc)); }
constexpr int64_t qtl_xbq_capacity(int64_t rows, int Pc) { return asc_xb_capacity(rows, qtl_cov_cols(Pc)); }
constexpr int64_t qtl_hitcount_capacity(int64_t rows) { return rows; }
constexpr int64_t qtl_rec_capacity(int64_t cap) { return 2 * cap; }
constexpr int64_t qtl_wsbest_blocks(int64_t rows, int64_t T) { return asc_row_blocks(rows) < qtl_chunk_blocks(T) ? asc_row_blocks(rows) : qtl_chunk_blocks(T); }
constexpr int64_t qtl_wsbest_capacity(int64_t rows, int64_t T) { return qtl_wsbest_blocks(rows, T) * T; }
constexpr int64_t qtl_wsbest_index(int64_t block, int64_t T, int64_t t) { return block * T + t; }
// the workgroup's static LDS: k_assoc's two stage buffers and sums at 64 columns, then per row mbar and sxx (f64), live and the hit
// count (u32), then the four waves' bests of a tile (r2 f64, row i64)
constexpr int64_t asc_lds_bytes(int nb, int ns) { return 2 * kAscRows * kAscGPitch + 2 * nb * 32 * kAscBPitch * 4 + kAscRows * ns * 4; }
constexpr int64_t qtl_lds_bytes() { return asc_lds_bytes(kQtlTile / 32, 3) + 2 * 8 * kAscRows + 2 * 4 * kAscRows + 4 * kQtlTile * 16; }
// The device bytes a call allocates (gpca_assoc_qtl's GPCA_ERR_OOM sum, without the check's slack)
constexpr double qtl_call_bytes(int64_t N, int64_t rows, int64_t T, int Pc, int64_t cap) {
    return 4.0 * (double)qtl_b_capacity(N, T) + 8.0 * (double)qtl_yy_capacity(T) + 4.0 * (double)qtl_q_capacity(N, Pc) + 4.0 * (double)asc_inc_capacity(N) +
           8.0 * (double)qtl_xbq_capacity(rows, Pc) + 4.0 * (double)asc_sums_capacity(rows) + 8.0 * (double)asc_info_capacity(rows) +
           4.0 * (double)qtl_hitcount_capacity(rows) + (4.0 + 8.0) * (double)qtl_rec_capacity(cap) + 16.0 * (double)qtl_wsbest_capacity(rows, T) +
           16.0 * (double)T + 8.0 /* the counter */ + 8.0 /* the invalid-genotype word */;
}

// ---- cis-QTL mapping (assoc_qtl_cis.hip, gpca_assoc_qtl_cis.cpp; include/gpca.h section a25) -------------------------------------------
// One trait at a time: its panel is the a24 panel of T = P + 1 columns (column 0 the residual, column p + 1 permutation p), built on the
// device by k_qtl_perm_panel, and its window [lo, hi) of kept rows goes through k_assoc_qtl_cis in launches of qtl_chunk_blocks(P + 1)
// row blocks that start at lo.  The per-row pass runs once over the union [ulo, uhi) of the windows.
constexpr int64_t kQtlCisMaxPerm = 65535;
// k_qtl_perm_panel: a workgroup of kQtlPermThreads threads owns qtl_perm_group(Pc) columns of the panel; in the first step a thread owns
// one (column, covariate) pair, in the second the threads walk the samples of one column after the other.  b_t sits in LDS up to
// kQtlPermLdsSamples included samples and is gathered from global memory above that.  Step 1 takes Q through LDS in tiles of
// kQtlPermQTile samples x Pc covariates.
constexpr int kQtlPermThreads = 256, kQtlPermLdsSamples = 4096, kQtlPermQTile = 32, kQtlPermQPitch = kQtlPermQTile + 1;
constexpr int qtl_perm_group(int Pc) { return Pc > 0 ? kQtlPermThreads / Pc : 16; }
static_assert(qtl_perm_group(kQtlMaxPc) >= 1 && qtl_perm_group(1) * 1 <= kQtlPermThreads, "a thread per (column, covariate) pair");
constexpr int64_t qtl_perm_grid(int64_t P, int Pc) { return (P + 1 + qtl_perm_group(Pc) - 1) / qtl_perm_group(Pc); }
// static LDS of k_qtl_perm_panel: b_t (f64), the group's c [columns][Pc] (f64; at most kQtlPermThreads pairs) and the tile of Q
// [kQtlMaxPc][kQtlPermQPitch] (f64) that step 1 reads
constexpr int64_t qtl_perm_lds_bytes() { return 8 * (int64_t)kQtlPermLdsSamples + 8 * (int64_t)kQtlPermThreads + 8 * (int64_t)kQtlMaxPc * kQtlPermQPitch; }
static_assert(qtl_perm_lds_bytes() <= 64 * 1024, "static LDS of k_qtl_perm_panel");
// the panel of one trait and where column `col` (0 = the residual, p + 1 = permutation p) of sample n sits in it
constexpr int64_t qtl_cis_panel_capacity(int64_t N, int64_t P) { return qtl_b_capacity(N, P + 1); }
constexpr int64_t qtl_cis_panel_index(int64_t col, int64_t npad, int64_t n) { return col * npad + n; }
// the call's resident inputs: the table [P][n] u32, Q [Pc][n] f64, the residuals of all traits [G][n] f64, S [n] i32
constexpr int64_t qtl_cis_table_capacity(int64_t P, int64_t n) { return P * n; }
constexpr int64_t qtl_cis_q_capacity(int Pc, int64_t n) { return (int64_t)Pc * n; }
constexpr int64_t qtl_cis_resid_capacity(int64_t G, int64_t n) { return G * n; }
constexpr int64_t qtl_cis_resid_index(int64_t g, int64_t n, int64_t i) { return g * n + i; }
// the bests of a launch: ws [row blocks][P + 1] (r2 f64, row i64) as a24's, and xb of column 0's best row per row block (f64)
constexpr int64_t qtl_cis_ws_blocks(int64_t rows, int64_t P) { return qtl_wsbest_blocks(rows, P + 1); }
constexpr int64_t qtl_cis_ws_capacity(int64_t rows, int64_t P) { return qtl_wsbest_capacity(rows, P + 1); }
constexpr int64_t qtl_cis_wsxb_capacity(int64_t rows, int64_t P) { return qtl_cis_ws_blocks(rows, P); }
// the running best of the trait in flight [P + 1] (r2 f64, row i64) and the results: perm_r2 [G][P] f64, column 0's [G][3] f64 =
// r2, xb, row (a kept row below 2^53 is exact in f64)
constexpr int64_t qtl_cis_run_capacity(int64_t P) { return P + 1; }
constexpr int64_t qtl_cis_result_capacity(int64_t G, int64_t P) { return G * P; }
constexpr int64_t qtl_cis_result_index(int64_t g, int64_t P, int64_t p) { return g * P + p; }
constexpr int64_t qtl_cis_best_capacity(int64_t G) { return 3 * G; }
// static LDS of k_assoc_qtl_cis: k_assoc_qtl's without the hit counts, plus the four waves' xb of column 0
constexpr int64_t qtl_cis_lds_bytes() { return asc_lds_bytes(kQtlTile / 32, 3) + 2 * 8 * kAscRows + 4 * kAscRows + 4 * kQtlTile * 16 + 4 * 8; }
static_assert(qtl_cis_lds_bytes() <= 64 * 1024, "static LDS of k_assoc_qtl_cis");
// The device bytes a call allocates (gpca_assoc_qtl_cis's GPCA_ERR_OOM sum, without the check's slack): rows = the union of the windows,
// wrows = the longest window
constexpr double qtl_cis_call_bytes(int64_t N, int64_t n, int64_t rows, int64_t wrows, int64_t G, int64_t P, int Pc) {
    return 4.0 * (double)qtl_cis_panel_capacity(N, P) + 4.0 * (double)qtl_cis_table_capacity(P, n) + 8.0 * (double)qtl_cis_q_capacity(Pc, n) +
           8.0 * (double)qtl_cis_resid_capacity(G, n) + 4.0 * (double)n + 4.0 * (double)qtl_q_capacity(N, Pc) + 4.0 * (double)asc_inc_capacity(N) +
           8.0 * (double)qtl_xbq_capacity(rows, Pc) + 4.0 * (double)asc_sums_capacity(rows) + 8.0 * (double)asc_info_capacity(rows) +
           16.0 * (double)qtl_cis_ws_capacity(wrows, P) + 8.0 * (double)qtl_cis_wsxb_capacity(wrows, P) + (16.0 + 8.0) * (double)qtl_cis_run_capacity(P) +
           8.0 * (double)qtl_cis_result_capacity(G, P) + 8.0 * (double)qtl_cis_best_capacity(G) + 8.0 /* the invalid-genotype word */;
}

}  // namespace gpca
