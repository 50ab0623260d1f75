// Launchers for the gfx950 kernels (kernels.hip).  Every launcher only enqueues work on `st`;
// none allocates or synchronises.  Shapes are validated by the callers in gpca_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "eig_result.h"  // the result block of the small dense step and the host's verdict on it, audited by tests/cpp/eig_result_audit.cpp
#include "plan_math.h"   // part counts, GEMM plans, workspace capacities: plain host arithmetic, audited by tests/cpp/plan_audit.cpp

namespace gpca {

struct QcParams { double min_call_rate, min_maf, max_hwe_p; };

// Kernel-selection switches of one handle (read from the environment at gpca_create; defaults = the measured best).
struct KernelOpts {
    int gq_phase = -1;   // workgroup b of k_gq_d starts its sweep of the sample axis at stage ((b % 8) A + (b / 8) B) mod stages, A = low 16 bits,
                         // B = high 16 bits; -1 = the launcher's choice (8 starting points per XCD up to 51k samples).  Harness knob.
    int gq_chain = 1;    // k_gq_d prefetches a wave's next round behind the current round's epilogue (0: drain + prologue per round).  Harness knob.
    int gtt_xcd = 1;     // XCD-aware workgroup order in k_gtt_d / k_gtt_p.  Harness knob.
};
// Opt-in to > 64 KiB of dynamic LDS for every kernel that needs it, on the CURRENT device (the attribute is per device).
// Return a hipError_t value (0 = ok).
int init_device_kernels_i8();
int init_device_kernels_common();
int init_device_kernels_eig();

// ---- the small dense step on the device (small_eig.hip) ----------------------------------------------------------------------
// (layout of the result block `res` of launch_small_eigh and the host's verdict on it: eig_result.h)
// Symmetric eigenproblem of the leading n x n block of W (pitch L; nslices > 0: W = the sum of `nslices` partial matrices [L * L] apart),
// symmetrised; descending.  Z [2][L][k]: zmode 0 -> Z0 = V_k diag(sv), Z1 = V_k diag(1 / sv); zmode 1 -> Z0 = Z1 = V_k.  Vout may be NULL.
void launch_small_eigh(hipStream_t st, const double* src, int nslices, int n, int L, int k, int zmode, double denom, const int* cholflag,
                       double* Z, double* res, double* Vout);

// C/D of a 32 x 32 MFMA: register e (0 .. 15) of a lane of half h (= lane >> 5) holds row (e & 3) + 8 (e >> 2) + 4 h of column
// lane & 31; acc_row = that row of the sub-tile whose first row is row0
template <class T>
__host__ __device__ inline constexpr T acc_row(T row0, int e, int h) { return row0 + (e & 3) + 8 * (e >> 2) + 4 * h; }

// Blocked layouts of the skinny GEMM operands (gemm_f32.hip): a lane's 8 / 16 k-steps are contiguous.
//   Tb [group = row/16][lt][lane = 32*(row&1) + col%32][u = (row%16)/2]      (8 floats per lane)
//   Qb [chunk = n/32][lt][lane = 32*((n%32)/16) + col%32][u = n%16]           (16 floats per lane)
__host__ __device__ inline int64_t blocked_t_index(int64_t row, int col, int LT) {
    const int64_t group = row >> 4;
    const int w = (int)(row & 15), lt = col >> 5, cc = col & 31;
    return ((group * LT + lt) * 64 + ((w & 1) * 32 + cc)) * 8 + (w >> 1);
}
__host__ __device__ inline int64_t blocked_q_index(int64_t n, int col, int LT) {
    const int64_t chunk = n >> 5;
    const int w = (int)(n & 31), lt = col >> 5, cc = col & 31;
    return ((chunk * LT + lt) * 64 + ((w >> 4) * 32 + cc)) * 16 + (w & 15);
}

void launch_synth(hipStream_t st, int8_t* G, int64_t M, int64_t N, int64_t ld, int64_t snp_offset,
                  uint64_t seed, const uint32_t* d_thresh, int P);
// Fast panel generator (GPCA_PANEL_SYNTH16): one 16-bit uniform per genotype (SplitMix64, counter mode), g = (u < t1) + (u < t2) with the 16-bit
// thresholds t2 = P(g = 2) (low half) and t1 = P(g >= 1) (high half) of thresh16[row][(n / 16) % P]; 4 genotypes per SplitMix64 output.
// packed = 0: int8 rows of pitch ld; 1: 2-bit dosage codes, rows of pitch ld bytes.  snp0 = global index of row 0.
void launch_synth16(hipStream_t st, void* G, int packed, int64_t rows, int64_t N, int64_t ld, int64_t snp0, uint64_t seed,
                    const uint32_t* d_thresh16, int P);
void launch_bed_decode(hipStream_t st, const uint8_t* bed, int64_t bytes_per_row, int8_t* G, int64_t M,
                       int64_t N, int64_t ld);
// a1: per-SNP {n_valid,n0,n1,n2}, mu, sigma, r = 1/sigma, b = -mu r, keep, reason; flags[0] |= 1 if any
// kept SNP holds a missing value, |= 2 if any kept SNP holds a value outside {0,1,2}.
void launch_snp_stats(hipStream_t st, const int8_t* G, int64_t M, int64_t N, int64_t ld, QcParams qc,
                      float* mu, float* sigma, float* r, float* b, uint8_t* keep, uint8_t* reason,
                      uint32_t* counts, uint32_t* flags);
// recompute r, b, flags from caller-supplied mu/sigma/keep (needs counts from a stats pass for the flags)
void launch_set_scale(hipStream_t st, int64_t M, const float* mu, const float* sigma, const uint8_t* keep,
                      float* r, float* b);
// a2: out[a][c] = fma((f32)g, 1/sigma, -mu/sigma); err_idx = min flat index of a missing genotype (or -1)
void launch_standardize_block(hipStream_t st, const int8_t* G, int64_t ld, const float* mu,
                              const float* sigma, const int64_t* rows, int64_t ns, const int64_t* cols,
                              int64_t nj, float* out, unsigned long long* err_idx);

// sketch operand: Tb (blocked, all Mpad rows) = r_i * Omega[i][j] (j < l, else 0); cpart[wave][j] = sum_i b_i Omega[i][j]
//   (omega_num_parts(Mpad) waves: plan_math.h)
// row_ids (may be NULL): global index of every row (a matrix of gathered rows draws the normals its rows would draw in place)
void launch_omega(hipStream_t st, int64_t M, int64_t Mpad, int l, int L, int64_t snp_offset, uint64_t seed,
                  const float* r, const float* b, float* Tb, float* cpart, double* apart, int blocked = 1, const int64_t* row_ids = nullptr);
void launch_gather_rows(hipStream_t st, const void* src, int64_t pitch, const int64_t* ids, int64_t n, void* dst);      // dst row i <- src row ids[i]
void launch_gather_elems(hipStream_t st, const void* src, int elem_bytes, const int64_t* ids, int64_t n, void* dst);   // 1-, 4- or 16-byte elements

// exact-integer path: the digit planes of T' = r o Omega directly (analytic column bound 6.67 * rmax[0]; no f32 T')
void launch_omega_planes(hipStream_t st, int64_t M, int64_t Mpad, int l, int L, int64_t snp_offset, uint64_t seed, const float* r,
                         const float* b, float* cpart, int8_t* Td, const float* rmax, double* tscale, double* tinv, int nd,
                         const int64_t* row_ids = nullptr);
// out[0] = max_i r[i] for r >= 0 (the caller zeroes out first)
void launch_max_f32(hipStream_t st, const float* r, int64_t n, float* out);

// K1: T = r o (G Q) + b s^T.  Tb != NULL: write r o T blocked into Tb and cpart[wave][j] = sum_i b_i T_ij
// (power iteration); Tb == NULL: write T row-major into Tout (projection B = A Q).  Qb is the blocked basis.
// (GqPlan / gq_plan: plan_math.h)
// G: int8 rows (packed = 0) or 2-bit dosage codes (packed = 1) of row pitch ldr bytes; Npad = padded sample count (multiple of 256)
void launch_gq_f32(hipStream_t st, const void* G, int packed, int64_t ldr, const GqPlan& plan, int64_t Npad, const float* Qb,
                   int L, const float* r, const float* b, const float* s, float* Tout, float* Tb, float* cpart);
// K2: Ypart[w][n][j] = 2^-9 * sum over the wave's SNP rows of G[i][n] * T'[i][j]   (T' blocked in Tb)
// (GttPlan / gtt_plan: plan_math.h)
void launch_gtt_f32(hipStream_t st, const void* G, int packed, int64_t ldr, int64_t Mpad, int64_t Npad, const float* Tb,
                    int L, float* Ypart, const GttPlan& plan);
// Y[n][j] = c[j] + 2^9 * sum_w Ypart[w][n][j]   (f64 sum), n < N
void launch_reduce_y(hipStream_t st, const float* Ypart, int W, int64_t Npad, int64_t N, int L, const double* c,
                     double* Y);

// generic tall-skinny helpers
// scratch: >= S * E doubles, S = sum_slices(P, E) <= 64 slices (<= 256 when E <= 64): sum_scratch_need(E) holds any part count
void launch_sum_partials_f32(hipStream_t st, const float* part, int64_t P, int64_t E, double* out, double* scratch);
void launch_sum_partials_f64(hipStream_t st, const double* part, int64_t P, int64_t E, double* out, double* scratch);
// slices of the part axis the first stage uses: sum_slices(P, E) (plan_math.h; a function of (P, E) only: the summation tree is the
// same for every run and partition)
#ifdef __HIPCC__
// The body of the two-stage sum (one workgroup of 256 threads = columns 64 bx .. + 63, slice by of S): out[by][e] = sum over the slice's
// parts in a fixed tree.  Shared by k_sum_partials and by the kernels that carry one of its stages along (k_post_k1, k_quantize).
template <typename T>
__device__ __forceinline__ void sum_partials_body(const T* __restrict__ part, int64_t P, int64_t E, double* __restrict__ out, int S, int bx, int by,
                                                  double (*red)[64]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t e = (int64_t)bx * 64 + lane;
    const int64_t per = (P + S - 1) / S;
    const int64_t p0 = by * per, p1 = (p0 + per < P) ? p0 + per : P;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (e < E) {
        int64_t p = p0 + wv;
        for (; p + 12 < p1; p += 16) {
            a0 += (double)part[p * E + e]; a1 += (double)part[(p + 4) * E + e];
            a2 += (double)part[(p + 8) * E + e]; a3 += (double)part[(p + 12) * E + e];
        }
        for (; p < p1; p += 4) a0 += (double)part[p * E + e];
    }
    red[wv][lane] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (wv == 0 && e < E) out[(int64_t)by * E + e] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}
#endif
// first stage only: *slices partial sums of [E] doubles at *src, for a consumer that folds the (<= 64, or <= 256 for E <= 64) slices
// itself (launch_small_eigh, k_chol_inv); P <= 64 parts are their own slices and nothing is launched
void launch_sum_partials_f64_stage1(hipStream_t st, const double* part, int64_t P, int64_t E, double* scratch, const double** src, int* slices);
// part [gram_num_parts(rows)][L * L]
void launch_gram_f64(hipStream_t st, const double* X, int64_t rows, int L, double* part);
void launch_gram_f32(hipStream_t st, const float* X, int64_t rows, int L, double* part);
// X[n][:] <- X[n][:] * Z  (Z: [L][L] f64, in place); optionally also the blocked f32 basis Qb (rows_pad rows, pad rows zeroed)
// the digit planes hold round(x * S / colmax): S = 0.49 * 128^4 keeps every digit of the signed base-128 expansion in int8
constexpr double kDigitScale = 0.49 * 268435456.0;
// three-plane mode (packed kernels only): round(x * S3 / colmax) in three signed base-256 digits, S3 = 0.49 * 256^3
constexpr double kDigitScale3 = 0.49 * 16777216.0;
inline double digit_scale(int nd) { return nd == 3 ? kDigitScale3 : kDigitScale; }
// last right-multiplication of CholeskyQR2 + partials of Q^T 1 and of the column abs-max; k_finish_q reduces them
// csum_part, amax_part [tail_num_parts(rows_pad)][L]
void launch_apply_right_tail(hipStream_t st, double* X, int64_t rows, int L, const double* Z, float* Qout, int64_t rows_pad,
                             double* csum_part, double* amax_part);
void launch_finish_q(hipStream_t st, const double* csum_part, const double* amax_part, int64_t P, int L, double* s64, float* s32,
                     double* scale, double* inv, int nd = 4);
// W = R^T R (n x n, pitch ld <= 64), Z = R^-1; *flag = j + 1 on a non-positive pivot (first failure wins)
int launch_chol_inv(hipStream_t st, const double* W, int n, int ld, double* Z, int* flag);      // a hipError_t value (0 = launched)
// the same from the Gram's P <= 64 partial sums [P][32 * 32] (ld = 32 only): the fold rides in front of the factorisation, no k_sum_partials launch
void launch_chol_inv_fold(hipStream_t st, const double* part, int P, int n, int ld, double* Z, int* flag);
void launch_apply_right_inplace(hipStream_t st, double* X, int64_t rows, int L, const double* Z, float* Qb,
                                int64_t rows_pad);
// out[n][kc] = sum_j X[n][j] Z[j][kc]   (Z: [L][K] f64)
void launch_rightmul_f64(hipStream_t st, const double* X, int64_t rows, int L, const double* Z, int K, double* out64,
                         float* out32);
// rows gathered through an index list (loadings of kept SNPs); sign (may be NULL): column c of Z is multiplied by sign[c]
void launch_rightmul_gather_f32(hipStream_t st, const float* X, const int64_t* row_ids, int64_t nrows, int L,
                                const double* Z, int K, float* out32, const int* sign = nullptr);
// Sample scores with their sign rule in two launches (L <= 64): launch_scores writes the unsigned scores X Z and, per workgroup and
// column, the first row with maximal |score| (value + row: scores_num_parts(rows) candidates); launch_scores_sign folds the candidates
// (every workgroup for itself: they are few), flips the columns whose winner is negative (in place, plus the f32 copy) and leaves
// sign[c] = +-1 for the loadings.
void launch_scores(hipStream_t st, const double* X, int64_t rows, int L, const double* Z, int K, double* out64, double* cand_val, int64_t* cand_idx);
void launch_scores_sign(hipStream_t st, double* out64, float* out32, int64_t rows, int K, const double* cand_val, const int64_t* cand_idx,
                        int64_t parts, int* sign);
// part [colsum_num_parts(rows)][L]
void launch_colsum_f64(hipStream_t st, const double* X, int64_t rows, int L, double* part);
// sign[c] = sign of the first element of column c with maximal |x|
void launch_col_sign(hipStream_t st, const double* X, int64_t rows, int K, int* sign);
void launch_scale_cols(hipStream_t st, double* X64, float* X32, int64_t rows, int K, const int* sign);
void launch_f64_to_f32(hipStream_t st, const double* in, float* out, int64_t n);
// exclusive scan of keep -> row list of kept SNPs (small M only needs one block; large M uses 2 passes)
void launch_fill_f32(hipStream_t st, float* p, int64_t n, float v);
// Tp[rows[a]][c] = load[a][c] for c < k (other entries untouched: caller zero-fills Tp first)
void launch_expand_loadings(hipStream_t st, const float* load, const int64_t* rows, int64_t n_pca, int k, int L, float* Tp);
// Tb (blocked, all Mpad rows) = r_i X[i][:]; cpart[wave][j] = sum over the wave's 64 rows of b_i X[i][j] (omega_num_parts(Mpad) waves)
void launch_scale_rows(hipStream_t st, const float* X, int64_t M, int64_t Mpad, int L, const float* r, const float* b,
                       float* Tb, float* cpart, int blocked = 1);


// EigenSNP stages: block-diagonal condensed basis W (kernels.hip)
void launch_bd_expand(hipStream_t st, const float* W, const int32_t* feat0, int cmax, const double* P, int64_t M, int L, float* out);
void launch_bd_reduce(hipStream_t st, const float* W, const int32_t* feat0, int cmax, const float* T, int L, const int64_t* blk_row0,
                      const int64_t* blk_row1, const int32_t* blk_feat0, const int32_t* blk_c, int B, double* P);
void launch_rightmul_inplace_f32(hipStream_t st, float* X, int64_t rows, int L, const double* Z);
void launch_mask_rows(hipStream_t st, double* Y, int64_t N, int L, const uint8_t* mask);
void launch_f32_to_f64(hipStream_t st, const float* in, double* out, int64_t n);

// ---- exact-integer path (gemm_i8.hip), 32 columns per launch.  Every K1 here writes cpart[unit][32] = the unit's share of
// b^T T (one partial per 32-row unit of the launch, partition-independent) and, except k_gq_i8, apart[wave][32] = column abs-max. ----------------------------------------------------------
constexpr int kDigits = 4;   // signed base-128 digits of the skinny operand
void launch_gq_i8(hipStream_t st, const int8_t* G, int64_t ldg, const GqPlan& plan, int64_t N, const int8_t* Qd,
                  const double* qscale, const float* r, const float* b, const float* s, float* Tout, float* cpart,
                  int scale_out, int64_t ldt = 32, const KernelOpts& ko = KernelOpts());
// K2 work decomposition: tasks = (row chunk, n-group) pairs -- an n-group is the 4 x 128 samples of a workgroup's four waves, a row chunk
// one of W near-equal ranges of the 128-row stages -- and every n-group ends with W partial tiles in Ypart[W][Npad][32].
// Simple kernels / narrow shapes: one task per workgroup (grid = tasks).  The DMA kernels (k_gtt_d, k_gtt_p) take `tasks_per_wg`
// CONSECUTIVE tasks per workgroup, n-group fastest, so that a launch is one batch of workgroups that end together: one task per
// workgroup ran 500 workgroups on 256 CUs at configs[1] and 392 at configs[3]'s shard -- a second, part-empty batch, 6 % and 14 % of
// the launch.  gtt8_plan_batched picks W (stages per task against per-task prologues, the fold's traffic and the L2 footprint of a
// row chunk's T' planes, which the workgroups of an XCD share).
// (Gtt8Plan and its three planners gtt8_plan, gtt8_plan_batched, gtt8_plan_narrow: plan_math.h)
void launch_gtt_i8(hipStream_t st, const int8_t* G, int64_t ldg, int64_t Mpad, int64_t Npad, const int8_t* Td,
                   double* Ypart, const Gtt8Plan& plan, const KernelOpts& ko = KernelOpts());
// narrow matrices (N <= 256 samples, int8 rows): every wave owns its own row range, Q's digit planes stay in registers (K1) /
// the four waves of a workgroup take four row chunks instead of four sample blocks (K2).  launch_gq_n returns a hipError_t value.
void launch_gtt_n(hipStream_t st, const int8_t* G, int64_t ldg, int64_t Mpad, int64_t Npad, const int8_t* Td, double* Ypart,
                  const Gtt8Plan& plan);
int launch_gq_n(hipStream_t st, const int8_t* G, int64_t ldg, const GqPlan& plan, int64_t N, const int8_t* Qd,
                const double* qscale, const float* r, const float* b, const float* s, float* Tout, float* cpart, double* apart,
                int scale_out, int64_t ldt = 32);
void launch_reduce_y_i8(hipStream_t st, const double* Ypart, int W, int64_t Npad, int64_t N, const double* c,
                        const double* tscale, double* Y, int64_t ldy = 32);
void launch_accum_y_i8(hipStream_t st, const double* Ypart, int W, int64_t Npad, int64_t N, double* Yint, int first);
void launch_finish_y_i8(hipStream_t st, const double* Yint, int64_t N, const double* c, const double* tscale, double* Y, int64_t ldy = 32);
void launch_absmax_fold(hipStream_t st, const double* apart, int64_t P, double* run);
void launch_accum_y_scaled(hipStream_t st, const double* Ypart, int W, int64_t Npad, int64_t N, const double* tscale, double* Yacc, int first);
void launch_finish_y_sum(hipStream_t st, const double* Yacc, int64_t N, const double* c, double* Y, int64_t ldy = 32);
// X [rows][32] row-major -> digit planes Xd [rows_pad/32][kDigits][64][16 B]; scale[j] = colmax_j / S, inv = 1/scale
// layout 0: 32 consecutive rows per block; layout 1: the MFMA-step order of the packed (2-bit) G Q kernel
void launch_quantize_f32(hipStream_t st, const float* X, int64_t rows, int64_t rows_pad, double* part, double* scale,
                         double* inv, int8_t* Xd, int layout = 0, int nd = 4, int64_t ldx = 32);
void launch_quantize_f64(hipStream_t st, const double* X, int64_t rows, int64_t rows_pad, double* part, double* scale,
                         double* inv, int8_t* Xd, int layout = 0, int nd = 4, int64_t ldx = 32);

// ---- 2-bit resident genotypes (store2bit.hip, gemm_i8.hip) -----------------------------------------------------
constexpr int64_t kSamplePad2bit = 1024;   // samples per row padded to this (ld2 = Npad / 4 bytes)
void launch_bed_to_codes(hipStream_t st, const uint8_t* bed, int64_t bpr, uint8_t* G2, int64_t M, int64_t N, int64_t ld2);
void launch_pack_i8(hipStream_t st, const int8_t* G8, int64_t ld8, uint8_t* G2, int64_t rows, int64_t N, int64_t ld2,
                    unsigned* flags);
void launch_snp_stats_2bit(hipStream_t st, const uint8_t* G2, int64_t M, int64_t N, int64_t ld2, QcParams qc, float* mu,
                           float* sigma, float* r, float* b, uint8_t* keep, uint8_t* reason, uint32_t* counts, uint32_t* flags);
void launch_standardize_block_2bit(hipStream_t st, const uint8_t* G2, int64_t ld2, const float* mu, const float* sigma,
                                   const int64_t* rows, int64_t ns, const int64_t* cols, int64_t nj, float* out,
                                   unsigned long long* err_idx);
void launch_gq_2bit(hipStream_t st, const uint8_t* G2, int64_t ld2, const GqPlan& plan, int64_t Npad, const int8_t* Qd,
                    const double* qscale, const float* r, const float* b, const float* s, float* Tout, float* cpart,
                    double* apart, int scale_out, int nd = 4, int64_t ldt = 32);
void launch_quantize_f64_prescaled(hipStream_t st, const double* X, int64_t rows, int64_t rows_pad, const double* inv, int8_t* Xd, int layout, int nd = 4, int64_t ldx = 32);
// the same with launch_finish_q folded in for these 32 columns (every workgroup folds the P abs-max partials itself: for P <= kFinishQFoldMax)
void launch_quantize_f64_finishq(hipStream_t st, const double* X, int64_t rows, int64_t rows_pad, int8_t* Xd, int layout, int nd, int64_t ldx,
                                 const double* csum_part, const double* amax_part, int64_t P, int ldp, double* s64, float* s32, double* scale, double* inv);
// quantise X whose column abs-max partials [P][32] were already produced by the kernel that wrote it (K1 epilogue)
void launch_quantize_f32_premax(hipStream_t st, const float* X, int64_t rows, int64_t rows_pad, const double* apart, int64_t P,
                                double* scale, double* inv, int8_t* Xd, int layout, int nd = 4, int64_t ldx = 32);
// What follows a K1 sweep of a power iteration, in two launches instead of four (resident matrices):
//   launch_post_k1:           first stage of c = b^T T over the units' partials cpart [units][32] (S = post_k1_slices(units) slices into
//                             cscratch) BESIDE the fold of the waves' column abs-max apart [P][32] into the digit scale (one more workgroup);
//   launch_quantize_f32_cfold: the digit planes of T' as launch_quantize_f32_premax's second half, and -- its first workgroup -- the
//                             second stage of c (cscratch -> c[32]).  Same summation tree as launch_sum_partials_f32: the same bits.
void launch_post_k1(hipStream_t st, const float* cpart, int64_t units, double* cscratch, const double* apart, int64_t P, double* scale, double* inv, int nd);
void launch_quantize_f32_cfold(hipStream_t st, const float* X, int64_t rows, int64_t rows_pad, const double* inv, int8_t* Xd, int layout, int nd,
                               int64_t ldx, const double* cscratch, int cslices, double* c);
// K2 for packed genotypes: stage-wise cooperative LDS-DMA (ring of four stage buffers); returns a hipError_t value
int launch_gtt_p(hipStream_t st, const uint8_t* G2, int64_t ld2, int64_t Mpad, int64_t Npad, const int8_t* Td, double* Ypart,
                 const Gtt8Plan& plan, int nd = 4, const KernelOpts& ko = KernelOpts());
// K2 with genotypes and digit planes brought in by LDS-DMA (int8-resident); returns a hipError_t value (0 = ok)
int launch_gtt_d(hipStream_t st, const int8_t* G, int64_t ldg, int64_t Mpad, int64_t Npad, const int8_t* Td, double* Ypart,
                 const Gtt8Plan& plan, const KernelOpts& ko = KernelOpts());
// K1 with the genotypes brought in by LDS-DMA (full-line pieces); returns a hipError_t value (0 = ok)
int launch_gq_d(hipStream_t st, const int8_t* G, int64_t ldg, const GqPlan& plan, int64_t Npad, const int8_t* Qd,
                const double* qscale, const float* r, const float* b, const float* s, float* Tout, float* cpart, double* apart,
                int scale_out, int64_t ldt = 32, const KernelOpts& ko = KernelOpts());
void launch_gtt_2bit(hipStream_t st, const uint8_t* G2, int64_t ld2, int64_t Mpad, int64_t Npad, const int8_t* Td,
                     double* Ypart, const Gtt8Plan& plan, int nd = 4);


// ---- projection onto a fitted model, missing calls mean-imputed (project.hip) ------------------------------------------------------
// Per 32-column half: Ypa / Ypb [W][Npad][32] = exact integer sums of g' (missing -> 0) against the digit planes Ta of r o W and of the
// missing indicator against the planes Tb of b o W (both in layout 0), one read of the genotypes; cnt[n] += missing calls of sample n in
// the rows whose bit is set in rmask [rows_pad / 32] (atomic, zeroed by the caller; cnt = NULL: not counted); *bad |= 1 when such a row holds a value outside
// {0, 1, 2, missing} (int8 rows).  lazy_b: the Tb planes are loaded only for blocks that hold a missing code (else with every
// block, in the register ring).  G: int8 rows (packed = 0) or 2-bit codes (packed = 1) of pitch ldr bytes.
// (PrjPlan / prj_plan: plan_math.h)
void launch_project(hipStream_t st, const void* G, int packed, int64_t ldr, int64_t Mpad, int64_t Npad, const int8_t* Ta, const int8_t* Tb,
                    const uint32_t* rmask, double* Ypa, double* Ypb, unsigned* cnt, unsigned* bad, const PrjPlan& plan, int nd, int lazy_b);
// Y[n][j] = fma(-tscale_b[j], Yint_b[n][j], Y[n][j])  (one 32-column half, pitch ldy); 0 for a sample with cnt[n] == n_model
void launch_project_correct(hipStream_t st, const double* Yint_b, int64_t N, const double* tscale_b, const unsigned* cnt, int64_t n_model,
                            double* Y, int64_t ldy);
// out[j] = max(out[j], max_i |X[i][j]|), X [rows][L] f32, out: the bits of non-negative doubles (zeroed by the caller)
void launch_project_colmax(hipStream_t st, const float* X, int64_t rows, int L, unsigned long long* out);
// used[n] = n_model - cnt[n]
void launch_project_used(hipStream_t st, const unsigned* cnt, int64_t N, double n_model, double* used);

// ---- genetic relationship matrix: lower-triangular SYRK over the kept rows (grm.hip) ---------------------------------------------------
// Tables of one 32-row block, kGrmTabBytes bytes: [4][kGrmDigits][32] base-128 digits (plane 0 least significant, each in [0, 127]) of
// w, 2w, c = -r b and e = b^2 on the call's common power-of-two scale (0 on rows that are not kept).  Integer partials are flushed to f64
// once per kGrmFlushRows rows, counted from the first row of the launch.
constexpr int kGrmDigits = 6;
constexpr int kGrmFlushRows = 4096;
constexpr int kGrmTabBytes = 4 * kGrmDigits * 32;
// tiles: (tile row, tile column) pairs of 64 x 64 output tiles, tile row >= tile column; R, Q: running sums of the band (first: from 0)
void launch_grm(hipStream_t st, const void* G, int packed, int64_t ldr, int64_t rows_pad, const int8_t* tab, const uint32_t* kmask,
                const int2* tiles, int64_t ntiles, int64_t row0, int64_t row1, int64_t N, double* R, int* Q, int first);
// Up, Vp [ceil(rows / kGrmFlushRows)][Npad]: per flush group, sum of qc g' and of qe m over kept rows; cnt += kept rows missing;
// *bad |= 1 on a kept row with a value outside {0, 1, 2, missing}
void launch_grm_vec(hipStream_t st, const void* G, int packed, int64_t ldr, int64_t rows, int64_t Npad, const uint8_t* keep,
                    const int64_t* qc, const int64_t* qe, double* Up, double* Vp, unsigned* cnt, unsigned* bad);
void launch_grm_vec_fold(hipStream_t st, const double* Up, const double* Vp, int64_t rows, int64_t Npad, double* u, double* v);
// out = S (R - u_a - u_b + beta - v_a - v_b), npairs (may be NULL) = K - cnt_a - cnt_b + Q, band rows [row0, row1)
void launch_grm_finish(hipStream_t st, const double* R, const int* Q, const double* u, const double* v, const unsigned* cnt, double S,
                       double beta, double K, int64_t row0, int64_t row1, double* out, double* npairs);

// ---- KING-robust kinship: lower-triangular SYRK of the het / missing / homozygous indicators over the kept rows (king.hip) ----------
// tiles: (tile row, tile column) pairs of 128 x 128 output tiles, tile row >= tile column; kmask: one bit per row (kept), per 32-row
// block of the launch; R [5][E]: running f64 sums XX, HH, HM, MH, MM of the band's strictly-lower entries (first: from 0)
void launch_king(hipStream_t st, const void* G, int packed, int64_t ldr, int64_t rows_pad, const uint32_t* kmask, const int2* tiles,
                 int64_t ntiles, int64_t row0, int64_t row1, int64_t N, double* R, int64_t E, int first);
// het[n], miss[n] += kept rows with a het / missing call (device u32); *bad |= 1 on a kept row with a value outside {0, 1, 2, missing}
void launch_king_vec(hipStream_t st, const void* G, int packed, int64_t ldr, int64_t rows, int64_t Npad, const uint8_t* keep,
                     unsigned* het, unsigned* miss, unsigned* bad);
// het_f, miss_f [Npad] = het, miss as f64 (the exchange buffer's slots)
void launch_king_vec_f64(hipStream_t st, const unsigned* het, const unsigned* miss, int64_t Npad, double* het_f, double* miss_f);
// kin [E] = the kinship of the band's pairs, counts (may be NULL) [E][3] = NSNP, HETHET, IBS0; band rows [row0, row1)
void launch_king_finish(hipStream_t st, const double* R, int64_t E, const double* het, const double* miss, double K, int64_t row0,
                        int64_t row1, double* kin, int* counts);

// ---- windowed LD: banded SYRK of the kept rows with themselves over the samples (ld.hip) ---------------------------------------------
// krows [K]: original row of every kept row; W [kLdProducts][(row1 - row0) * wmax] i32 product planes, zeroed by the caller; weff: the
// widest window of the band in slots (tiles beyond it are not multiplied)
void launch_ld(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t K, int64_t N, int64_t row0,
               int64_t row1, const int64_t* win_end, int wmax, int weff, int* W);
// stat [hi - row0][3] = sum g', sum g'^2, missing calls of kept rows [row0, hi); *bad = min original row with a value outside
// {0, 1, 2, missing} (left as it is when there is none)
void launch_ld_vec(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t N, int64_t row0, int64_t hi,
                   unsigned* stat, unsigned long long* bad);
// r2 [rows][wmax], counts [rows][wmax][6], above [rows][ld_above_words(wmax)] (each may be NULL) from the planes and the per-row sums
void launch_ld_finish(hipStream_t st, const int* W, const unsigned* stat, int64_t N, int64_t row0, int64_t row1, const int64_t* win_end,
                      int wmax, double threshold, double* r2, int* counts, unsigned long long* above);
// LD scores from the same planes and per-row sums (stat holds rows [row0, hi)): acc [ld_score_span] i64 += rint(v 2^40) of every counted
// pair at its row and at its partner, partners [ld_score_span] i32 += 1 at the same two places; both zeroed by the caller
void launch_ld_score(hipStream_t st, const int* W, const unsigned* stat, int64_t N, int64_t row0, int64_t row1, int64_t hi,
                     const int64_t* win_end, int wmax, int weff, int unbiased, long long* acc, int* partners);

// ---- PC-Relate: regression of the kept rows on the PCs, then an f32 lower-triangular SYRK over the kept rows (pcrelate.hip) ----------
// krows [K]: original row of every kept row.  Hw [kPcrBetaWaves][N][width] f64: the hat matrix, coefficient j = wave * width + q (zero
// columns for samples outside the training set and for j > P); train [N].  betaG [pcr_kpad(K) / 8][P + 1][8] f32 (rows past K: 0),
// beta_rm (may be NULL) [K][P + 1]; *bad = min original row with a value outside {0, 1, 2, missing} (left as it is when there is none)
void launch_pcrelate_beta(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t K, int64_t N,
                          const uint8_t* train, const double* Hw, int P, float* betaG, float* beta_rm, unsigned long long* bad);
// mu [(row1 - row0)][N] f32: the individual-specific allele frequency of kept rows [row0, row1); X [pcr_npad(N)][P + 1] f32
void launch_pcrelate_isaf(hipStream_t st, const float* betaG, const float* X, int P, int64_t N, int64_t row0, int64_t row1, float* mu);
// inv[n] += kept rows where sample n's entry is invalid (missing, or mu outside (tau, 1 - tau)); inv zeroed by the caller
void launch_pcrelate_inv(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t K, int64_t N,
                         const float* betaG, const float* X, int P, float tau, unsigned* inv);
// tiles: (tile row, tile column) pairs of 128 x 128 output tiles, tile row >= tile column; R [2][E] f64: num, den of the band's
// entries (diagonal included); Q [E]: kept rows where both entries are invalid
int launch_pcrelate(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t K, int64_t N, const float* betaG,
                    const float* X, int P, float tau, const int2* tiles, int64_t ntiles, int64_t row0, int64_t row1, double* R, int* Q, int64_t E);
// kin [E] = num / (4 den) (NaN when nsnp = 0), nsnp (may be NULL) [E] = K - inv_a - inv_b + Q; band rows [row0, row1)
void launch_pcrelate_finish(hipStream_t st, const double* R, const int* Q, const unsigned* inv, int64_t K, int64_t E, int64_t row0,
                            int64_t row1, double* kin, int* nsnp);

// ---- linear association scan: kept rows x (traits + covariates) over the samples, missing calls mean-imputed (assoc.hip) -------------
// krows: original row of every kept row.  Bt [asc_lpad(L)][asc_npad(N)] f32 (zero past N and past L); incw: the include mask, one bit
// per sample (asc_inc_capacity(N) words, zero past N).  xb [row1 - row0][L] f64 = d + mbar e; sums [row1 - row0][3] u32 = n_obs, sum g',
// sum g'^2; *bad = min original row with a value outside {0, 1, 2, missing} (left as it is when there is none)
int launch_assoc(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t N, const float* Bt,
                 const unsigned* incw, int L, int64_t row0, int64_t row1, double* xb, unsigned* sums, unsigned long long* bad);
// stats [rows][T][3] = beta, se, t and info [rows][4] = n_obs, a1_freq, xx, sxx (each may be NULL); yy [T]
void launch_assoc_finish(hipStream_t st, const double* xb, const unsigned* sums, const double* yy, int T, int L, double df, double max_vif,
                         int64_t rows, double* stats, double* info);

// ---- many-trait QTL scan: kept rows x a strip of trait columns per workgroup, thresholded in the epilogue (assoc_qtl.hip) -------------
// One launch covers the kept rows [row0, row1) of the band that starts at band0 (row0 - band0 a multiple of kAscRows, at most
// qtl_chunk_blocks(T) row blocks).  Bt [qtl_tpad(T)][asc_npad(N)] f32 and yy [qtl_tpad(T)]; sums, info: launch_assoc's and
// launch_assoc_finish's of the band on the covariate basis; tw: a legal strip width (qtl_clamp_tw).  hit_count [band rows] u32 and
// *counter (u64) are added to (integer atomics); a hit's record goes to hit_index [cap][2] (kept row, trait) / hit_value [cap][2] (xb, r2)
// at the counter's value, dropped at or past cap; ws_r2 / ws_row [row blocks of the launch][T] = the workgroups' best (r2, kept row) per
// trait, (-1, -1) without a live row
int launch_assoc_qtl(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t N, const float* Bt,
                     const unsigned* incw, const double* yy, int64_t T, int tw, int64_t band0, int64_t row0, int64_t row1, const unsigned* sums,
                     const double* info, double max_vif, double r2_min, unsigned* hit_count, unsigned* hit_index, double* hit_value, int64_t cap,
                     unsigned long long* counter, double* ws_r2, long long* ws_row);
// folds ws [blocks][T] into the running best [T] (r2 = -1, row = -1: none yet): blocks ascending, replaced on a strictly larger r2
void launch_assoc_qtl_best(hipStream_t st, const double* ws_r2, const long long* ws_row, int64_t blocks, int64_t T, double* best_r2,
                           long long* best_row);

// ---- cis-QTL mapping: the permuted panel of one trait, its window scanned for the best row of every column (assoc_qtl_cis.hip) ---------
// out [P + 1][npad] f32 (zeroed by the caller where no included sample sits): column 0 = (float) b, column p + 1 = (float) of b gathered
// through perm [p] and taken back into the complement of Qt [Pc][n] (f64); b [n] f64; S [n] = the sample of i (NULL: i itself)
void launch_qtl_perm_panel(hipStream_t st, const double* b, const double* Qt, int Pc, int64_t n, const uint32_t* perm, int64_t P, const int* S,
                           int64_t npad, float* out);
// One launch covers the kept rows [row0, row1) (at most qtl_chunk_blocks(T) row blocks from row0) of a window inside the band that starts
// at band0; T = P + 1 columns of Bt [qtl_tpad(T)][asc_npad(N)], all with the trait's yy; sums, info as launch_assoc_qtl.  ws_r2 / ws_row
// [row blocks][T] and ws_xb [row blocks] = the workgroups' best (r2, kept row) per column and xb of column 0's
int launch_assoc_qtl_cis(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t N, const float* Bt,
                         const unsigned* incw, double yy, int64_t T, int tw, int64_t band0, int64_t row0, int64_t row1, const unsigned* sums,
                         const double* info, double max_vif, double* ws_r2, long long* ws_row, double* ws_xb);
// folds the launch into the trait's running best (first: starts it); last: writes perm_r2 [g][T - 1] and best [g][3] = r2, xb, row
void launch_assoc_qtl_cis_best(hipStream_t st, const double* ws_r2, const long long* ws_row, const double* ws_xb, int64_t blocks, int64_t T,
                               int first, int last, double* run_r2, long long* run_row, double* run_xb, int64_t g, double* perm_r2, double* best);

// ---- logistic score scan: kept rows x T (Pc + 3) panel columns over the samples, the operand coded by the minor allele (assoc_score.hip)
// sums [row1 - row0][3] u32 = n_obs, sum g o, sum g^2 o; *bad as in launch_assoc
int launch_assoc_score_count(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t N, const unsigned* incw,
                             int64_t row0, int64_t row1, unsigned* sums, unsigned long long* bad);
// Bt [asc_lpad(L)][asc_npad(N)] f32, L = T (Pc + 3), columns in the order of asr_col_* (plan_math.h); sums: the count kernel's, same band;
// dv [row1 - row0][L] f64 = d + xbar e, and q + xbar^2 e in the w columns
int launch_assoc_score(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t N, const float* Bt,
                       const unsigned* incw, int T, int L, int64_t row0, int64_t row1, const unsigned* sums, double* dv);
// stats [rows][T][5] = beta, se, z, vw, V; ua [rows][T][Pc + 3] = U, gwg, a_0 .. a_Pc; info [rows][5] = n_obs, a1_freq, xx, flipped, 0
// (each may be NULL)
void launch_assoc_score_finish(hipStream_t st, const double* dv, const unsigned* sums, int T, int Pc, double max_vif, int64_t rows,
                               double* stats, double* ua, double* info);

// ---- saddle-point correction of the score scan (assoc_spa.hip): the items [item0, item0 + nitems) of a band (item = row T + trait)
// out [rows][T][4] = the normal -log10 p, status 0, NaN, NaN; list [*count] = the items with finite |z| >= spa_z and U != 0, relative to
// item0, in any order (*count is zero on entry; stats, dv: what the score kernels left for the band)
void launch_assoc_spa_flag(hipStream_t st, const double* stats, const double* dv, int T, int Pc, int64_t item0, int64_t nitems, double spa_z,
                           double* out, int* list, unsigned* count);
// the listed items' out = -log10 p, status, zeta+, zeta-; Z [T][Pc + 1][asp_gpad(N)] and mu [T][asp_gpad(N)] f64, 0 outside the included
// samples; gws: asp_g_capacity(N) doubles; row0: the band's first kept row; slots: the workgroups of the launch, 1 .. asp_slots(N) (refused
// outside: asp_clamp_slots), which decide only which workgroup computes an item
int launch_assoc_spa(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t N, const unsigned* incw,
                     const unsigned* sums, const double* dv, const double* Z, const double* mu, int T, int Pc, int64_t row0, int64_t item0,
                     const int* list, const unsigned* count, double* gws, double* out, int64_t slots);

// ---- Firth correction of the score scan (assoc_firth.hip): the same ranges, list and buffers as the saddle-point correction's
// out [rows][T][kAfiWidth] = the normal -log10 p, status 0, NaN, NaN, NaN; list [*count] = the items with finite |z| >= firth_z
void launch_assoc_firth_flag(hipStream_t st, const double* stats, int T, int64_t item0, int64_t nitems, double firth_z, double* out, int* list,
                             unsigned* count);
// the listed items' out = -log10 p, status, beta of A1, se, D; the arguments are launch_assoc_spa's
int launch_assoc_firth(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t N, const unsigned* incw,
                       const unsigned* sums, const double* dv, const double* Z, const double* mu, int T, int Pc, int64_t row0, int64_t item0,
                       const int* list, const unsigned* count, double* gws, double* out, int64_t slots);

// ---- gene-level set tests of the score scan (assoc_set.hip): lrows [listed] = the listed rows' original rows, sums and dv = what the
// score scan's kernels left for them (band = the list), strips [n_strips] (plan_math.h: AsgStrip), phi [tri_total][T] as asg_phi_index
// says.  The Gram kernel leaves R_ab, the finish kernel turns it into Phi_ab in place.
int launch_assoc_set_gram(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* lrows, int64_t N, const float* Bt,
                          const unsigned* incw, int T, const unsigned* sums, const AsgStrip* strips, int64_t n_strips, double* phi);
int launch_assoc_set_finish(hipStream_t st, const double* dv, const unsigned* sums, int T, int Pc, const AsgStrip* strips, int64_t n_strips,
                            double* phi);

// ---- per-group genotype counts (group_counts.hip): O [gc_ppad(P)][gc_npad(N)] = the one-hot matrix of the labels group [N] (-1: no
// group), size [P] = the samples of each group; counts [row1 - row0][P][3] u32 = n_obs, n_het, n_hom2 of kept rows [row0, row1) (PCA-SNP
// order through krows); *bad as in launch_assoc
void launch_gc_onehot(hipStream_t st, const int32_t* group, int64_t N, int P, uint8_t* O);
int launch_group_counts(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t N, const uint8_t* O,
                        const unsigned* size, int P, int64_t row0, int64_t row1, unsigned* counts, unsigned long long* bad);

// ---- f2 jackknife blocks (f2_blocks.hip): counts [rows][P][3] as launch_group_counts leaves them, block [rows] in -1 .. B - 1 (-1: the
// row enters nothing); acc [B][pairs] i64 += rint(v 2^40) and cnt [B][pairs] i32 += 1 of every (row, pair) with both groups observed,
// both zeroed by the caller.  Nonzero when P or rows is outside the kernel's limits (plan_math.h: fb_*).
int launch_f2_blocks(hipStream_t st, const unsigned* counts, const int* block, int64_t rows, int P, long long* acc, int* cnt);

// ---- per-sample genotype counts (sample_counts.hip): part [plan.splits][sc_npad(N)][3] u32 = missing, het, hom2 and (q given)
// qpart [plan.splits][sc_npad(N)] u64 = the q of the missing calls, per row split of kept rows [row0, row1) (PCA-SNP order through
// krows; q [row1 - row0]); *bad as in launch_assoc.  launch_sc_sum: counts [N][3] = n_obs, n_het, n_hom2 and qsum [N] = qtot - the
// missing calls' q (qpart and qsum NULL: counts alone)
int launch_sample_counts(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t N, const unsigned* q,
                         int64_t row0, int64_t row1, const ScPlan& plan, unsigned* part, unsigned long long* qpart,
                         unsigned long long* bad);
void launch_sc_sum(hipStream_t st, const unsigned* part, const unsigned long long* qpart, int64_t N, int64_t splits, int64_t rows,
                   unsigned long long qtot, unsigned* counts, unsigned long long* qsum);

// ---- runs of homozygosity (roh.hip) over kept rows [row0, row1) (PCA-SNP order through krows), all N samples; extents: plan_math.h roh_*.
// launch_roh_mark: plane [rows][roh_plane_pitch(N)] = the in-ROH bit of every (row, sample); dom [domains + 1] = the band-relative first
// rows of the window domains, then rows; window W, at most H het and M missing calls per hit, a row is in iff hits den >= num cov; *bad
// as in launch_assoc.  launch_roh_runs (k_roh_runs, then k_roh_stitch): segs NULL = the count pass (rec [plan.splits][roh_npad(N)][8] =
// what crosses the split boundaries; cnt [plan.splits][roh_npad(N)] = per sample the records of the splits before; seg_count [N] = the
// reported runs); else the fill pass (rec and cnt as the count pass left them, base [N] = the records of the samples before,
// segs [cap][5]).  brk [rows]: bit 1 = a run may not continue into the row.  The launches return nonzero when an argument is outside the
// kernels' limits.
int launch_roh_mark(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t N, int64_t row0, int64_t row1,
                    const RohPlan& plan, const int* dom, int64_t domains, int W, int H, int M, int num, int den, uint8_t* plane,
                    unsigned long long* bad);
int launch_roh_runs(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t N, int64_t row0, int64_t row1,
                    const RohPlan& plan, const uint8_t* brk, const uint8_t* plane, int64_t min_snp, int64_t max_het, unsigned* rec,
                    unsigned* cnt, unsigned* seg_count, const unsigned long long* base, unsigned* segs, int64_t cap);

// ---- admixture proportions (admix.hip; include/gpca.h section a21) over all `rows` kept rows (PCA-SNP order through krows) and all N
// samples; extents: plan_math.h adm_*.  Q [N][K], F [rows][K] f32; mode [N] or NULL.  launch_admix_step: one EM step (k_admix_step, then
// the slab sums with the F and Q updates and the sum of the log-likelihood terms): Qn, Fn and *ll (device f64); *bad as in launch_assoc.
// launch_admix_init: a21's init from counts [M][4] (the QC counts of every row).  launch_admix_norms: nrm [2] = sum r^2, sum v^2 over Q and
// F of three parameter sets.  launch_admix_extrap: (Qx, Fx) = the SQUAREM point of step length alpha, clamped.  The launches return
// nonzero when an argument is outside the kernels' limits.
struct AdmSet { float* Q; float* F; };
// a22's hold-out: folds = 0 is the plain step (llpart [partial], ll [1]); folds 2 .. 64 masks the observed calls of fold `fold` under `seed`
// (llpart [partial][2], ll [2] = loglik, held_loglik; counts [2] (device u64) += n_held, n_het_held: the caller zeroes them)
struct AdmHold { int folds = 0, fold = 0; uint64_t seed = 0; unsigned long long* counts = nullptr; };
int launch_admix_step(hipStream_t st, const void* G, int packed, int64_t ldr, const int64_t* krows, int64_t rows, int64_t N, int K,
                      const float* Q, const float* F, const uint8_t* mode, float* fpart, float* qpart, double* llpart, float* Qn, float* Fn,
                      double* ll, unsigned long long* bad, const AdmHold& hold = AdmHold{});
int launch_admix_init(hipStream_t st, const int64_t* krows, const unsigned* counts, int64_t rows, int64_t N, int K, uint64_t seed, float* Q,
                      float* F);
int launch_admix_norms(hipStream_t st, int64_t rows, int64_t N, int K, const AdmSet& t0, const AdmSet& t1, const AdmSet& t2, double* npart,
                       double* nrm);
int launch_admix_extrap(hipStream_t st, int64_t rows, int64_t N, int K, const AdmSet& t0, const AdmSet& t1, const AdmSet& t2,
                        const uint8_t* mode, double alpha, const AdmSet& tx);

}  // namespace gpca
