// Host-side audit of genomic_pca_amd/csrc/plan_math.h: for every sketch width and a grid of row and sample counts,
//   (1) every writer's extent is at most the capacity of the buffer it writes,
//   (2) every plan covers every row and every sample exactly once, with no index past Mpad / Npad,
//   (3) every count that one workgroup folds respects the limit its kernel documents.
// Plain C++: g++ -I genomic_pca_amd/csrc plan_audit.cpp.  Prints one line per violation ("FAIL ...") and a summary; exit status 1 on
// any violation.  tests/test_plan_audit.py builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstdarg>
#include <cstdint>
#include <vector>
#include <map>
#include <string>
#include <algorithm>
#include "plan_math.h"

using namespace gpca;

static long g_fail = 0, g_checks = 0;
static std::map<std::string, int> g_printed;
static void fail(const char* fmt, ...) {
    ++g_fail;
    char line[512];
    va_list ap; va_start(ap, fmt);
    std::vsnprintf(line, sizeof line, fmt, ap);
    va_end(ap);
    const std::string text(line);
    if (g_printed[text]++ || ++g_printed[text.substr(0, text.find(':'))] > 4) return;      // (the first lines of every kind tell the story)
    std::printf("FAIL %s\n", line);
}
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) fail(__VA_ARGS__); } while (0)

static int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

// SplitMix64: the seeded grid is the same on every machine
static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// values 1 .. hi: the edges the kernels are built on, and `nrand` seeded draws, log-uniform (small and large counts alike)
static std::vector<int64_t> grid(int64_t hi, int nrand) {
    const int64_t edges[] = {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193,
                             16384, 16385, 65536, 262143, 262144, 262145, 294912, 294913, 1000000, 2097151, 2097152, 2097153, 4194303,
                             4194304, 4194305, 10000000, 33554432, 100000000};
    std::vector<int64_t> v;
    for (int64_t e : edges) if (e <= hi) v.push_back(e);
    v.push_back(hi);
    for (int i = 0; i < nrand; ++i) {
        const int bits = 1 + (int)(next_u64() % 27);                      // up to 2^27 > 1e8
        int64_t x = (int64_t)(next_u64() & (((uint64_t)1 << bits) - 1)) | ((int64_t)1 << (bits - 1));
        if (x > hi) x = 1 + (int64_t)(next_u64() % (uint64_t)hi);
        v.push_back(x);
    }
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    return v;
}

// ---- the two-stage sum: sum_partials_body (kernels.h) gives slice `by` the parts [by * per, min(P, (by + 1) * per)), per = ceil(P / S) --------
static void check_sum(const char* who, int L, const char* dim, int64_t n, int64_t P, int64_t E, int64_t capacity, bool folded_by_one_workgroup) {
    const int S = sum_slices(P, E);
    CHECK(S >= 1, "%s: L=%d %s=%lld: sum_slices(%lld, %lld) = %d", who, L, dim, (long long)n, (long long)P, (long long)E, S);
    if (S > 1)      // (S == 1: the single stage writes `out`, not the scratch)
        CHECK((int64_t)S * E <= capacity, "%s: L=%d %s=%lld: parts=%lld S=%d writes %lld doubles into a buffer of %lld", who, L, dim, (long long)n,
              (long long)P, S, (long long)((int64_t)S * E), (long long)capacity);
    const int64_t per = (P + S - 1) / S;
    CHECK(per * S >= P, "%s: L=%d %s=%lld: %d slices of %lld parts do not cover %lld parts", who, L, dim, (long long)n, S, (long long)per, (long long)P);
    if (folded_by_one_workgroup) {
        // the consumer (launch_small_eigh, k_chol_inv, k_quantize's c fold) folds the slices itself: <= 64, or <= 256 for E <= 64;
        // S == 1 hands it the P parts themselves
        const int64_t slices = S == 1 ? P : S, lim = E <= 64 ? kSumSlicesMaxNarrow : kSumSlicesMax;
        CHECK(slices <= lim, "%s: L=%d %s=%lld: the consumer folds %lld slices, its limit is %lld", who, L, dim, (long long)n, (long long)slices, (long long)lim);
    }
}

// row chunks [w * rpw, min(Mpad, (w + 1) * rpw)), w < W: a partition of [0, Mpad) into non-empty pieces that are multiples of `gran`
static void check_chunks(const char* who, int64_t Mpad, int64_t Npad, int64_t W, int64_t rpw, int64_t gran) {
    CHECK(W >= 1 && rpw >= gran && rpw % gran == 0, "%s: Mpad=%lld Npad=%lld: W=%lld rows_per_wave=%lld (granule %lld)", who, (long long)Mpad,
          (long long)Npad, (long long)W, (long long)rpw, (long long)gran);
    CHECK(W * rpw >= Mpad, "%s: Mpad=%lld Npad=%lld: %lld chunks of %lld rows leave rows uncovered", who, (long long)Mpad, (long long)Npad, (long long)W, (long long)rpw);
    CHECK((W - 1) * rpw < Mpad, "%s: Mpad=%lld Npad=%lld: chunk %lld starts at row %lld, past Mpad", who, (long long)Mpad, (long long)Npad, (long long)(W - 1),
          (long long)((W - 1) * rpw));
}
// n-groups of 4 blocks of `blk` samples: block (g * 4 + wv) * blk < Npad is live; every block of [0, Npad) belongs to exactly one group
static void check_ngroups(const char* who, int64_t Mpad, int64_t Npad, int64_t ngroups, int64_t blk) {
    CHECK(Npad % blk == 0, "%s: Npad=%lld is not a multiple of the %lld-sample block", who, (long long)Npad, (long long)blk);
    CHECK(ngroups * 4 * blk >= Npad && (ngroups - 1) * 4 * blk < Npad, "%s: Mpad=%lld Npad=%lld: %lld n-groups of %lld samples", who, (long long)Mpad,
          (long long)Npad, (long long)ngroups, (long long)(4 * blk));
}

// the walk of k_gtt_d / k_gtt_p over its tasks (K2Walk, gemm_i8.hip), replayed: every (row chunk, n-group) exactly once
static void check_batched_walk(const Gtt8Plan& p, int64_t Mpad, int64_t Npad) {
    const int64_t T = (int64_t)p.W * p.ngroups;
    CHECK(p.grid * p.tasks_per_wg >= T && p.grid >= 1 && p.tasks_per_wg >= 1, "gtt8_plan_batched: Mpad=%lld Npad=%lld: grid %lld x %d tasks < %lld tasks",
          (long long)Mpad, (long long)Npad, (long long)p.grid, p.tasks_per_wg, (long long)T);
    if (T > 300000) return;                                   // (the arithmetic above covers the large shapes; the replay the rest)
    std::vector<unsigned char> seen((size_t)T, 0);
    long bad = 0;
    for (int64_t v = 0; v < p.grid; ++v) {
        const int64_t t_first = p.strided ? v : v * p.tasks_per_wg, t_step = p.strided ? p.grid : 1;
        int ntask = 0;
        if (t_first < T) { const int64_t left = (T - 1 - t_first) / t_step + 1; ntask = (int)(left < p.tasks_per_wg ? left : p.tasks_per_wg); }
        int64_t wch = t_first / p.ngroups, g = t_first - wch * p.ngroups;
        const int64_t wch_step = t_step / p.ngroups, g_step = t_step - wch_step * p.ngroups;
        for (int i = 0; i < ntask; ++i) {
            if (wch < 0 || wch >= p.W || g < 0 || g >= p.ngroups || wch * p.C >= p.S) { ++bad; break; }
            unsigned char& s = seen[(size_t)(wch * p.ngroups + g)];
            if (s) ++bad;
            s = 1;
            wch += wch_step; g += g_step; if (g >= p.ngroups) { g -= p.ngroups; ++wch; }
        }
    }
    for (unsigned char s : seen) if (!s) ++bad;
    CHECK(bad == 0, "gtt8_plan_batched: Mpad=%lld Npad=%lld: W=%d ngroups=%lld grid=%lld tasks_per_wg=%d: %ld tasks missed, repeated or out of range",
          (long long)Mpad, (long long)Npad, p.W, (long long)p.ngroups, (long long)p.grid, p.tasks_per_wg, bad);
}

static void audit_plans(int64_t M, int64_t N, int packed, int gq_target, int gtt_target) {
    const int64_t Mpad = round_up(M, kGQRowsPerWave), Npad = round_up(N, packed ? 1024 : kSamplePad);
    // K1: wave w owns the units [units * w / waves, units * (w + 1) / waves)
    const GqPlan gq = gq_plan(Mpad, gq_target);
    CHECK(gq.units * 32 == Mpad && gq.waves >= 4 && gq.waves % 4 == 0, "gq_plan: Mpad=%lld: units=%lld waves=%lld", (long long)Mpad, (long long)gq.units, (long long)gq.waves);
    CHECK(gq.waves <= std::max<int64_t>(4, round_up(std::min<int64_t>(gq.units, gq_target), 4)), "gq_plan: Mpad=%lld: %lld waves", (long long)Mpad, (long long)gq.waves);
    // (the ranges telescope by construction; what the kernels rely on: the products units * wave fit, and gemm_i8.hip casts a unit index to int)
    CHECK(gq.units < ((int64_t)1 << 31) && gq.units <= INT64_MAX / (gq.waves + 1), "gq_plan: Mpad=%lld: units=%lld waves=%lld overflow the unit ranges", (long long)Mpad, (long long)gq.units, (long long)gq.waves);
    // K2, f32 path
    {
        const GttPlan p = gtt_plan(Mpad, Npad, 32, gtt_target);
        check_chunks("gtt_plan", Mpad, Npad, p.W, p.rows_per_wave, 32);
        CHECK(p.nblocks_n * kSamplePad == Npad && p.grid == (p.nblocks_n + 3) / 4 * p.W, "gtt_plan: Mpad=%lld Npad=%lld: grid", (long long)Mpad, (long long)Npad);
        check_ngroups("gtt_plan", Mpad, Npad, (p.nblocks_n + 3) / 4, kSamplePad);
    }
    // K2, exact path: simple kernels, DMA kernels, narrow kernel; a task's i32 accumulators hold at most 2^22 rows
    {
        const Gtt8Plan p = gtt8_plan(Mpad, Npad, gtt_target);
        check_chunks("gtt8_plan", Mpad, Npad, p.W, p.rows_per_wave, 128);
        check_ngroups("gtt8_plan", Mpad, Npad, (p.nblocks_n + 3) / 4, 128);
        CHECK(p.grid == (p.nblocks_n + 3) / 4 * p.W, "gtt8_plan: Mpad=%lld Npad=%lld: grid", (long long)Mpad, (long long)Npad);
        CHECK(p.rows_per_wave <= ((int64_t)1 << 22), "gtt8_plan: Mpad=%lld Npad=%lld: %lld rows in one i32 accumulation", (long long)Mpad, (long long)Npad, (long long)p.rows_per_wave);
    }
    {
        const Gtt8Plan p = gtt8_plan_batched(Mpad, Npad, gtt_target);
        CHECK(p.S * 128 == Mpad && p.C >= 1, "gtt8_plan_batched: Mpad=%lld Npad=%lld: S=%lld C=%lld", (long long)Mpad, (long long)Npad, (long long)p.S, (long long)p.C);
        check_chunks("gtt8_plan_batched", Mpad, Npad, p.W, p.C * 128, 128);
        check_ngroups("gtt8_plan_batched", Mpad, Npad, p.ngroups, 128);
        CHECK(p.C * 128 <= ((int64_t)1 << 22), "gtt8_plan_batched: Mpad=%lld Npad=%lld: %lld rows in one i32 accumulation", (long long)Mpad, (long long)Npad, (long long)(p.C * 128));
        check_batched_walk(p, Mpad, Npad);
    }
    if (!packed && N <= kNarrowSamples) {
        const Gtt8Plan p = gtt8_plan_narrow(Mpad, N, std::min(gtt_target, 1024));
        check_chunks("gtt8_plan_narrow", Mpad, Npad, p.W, p.rows_per_wave, 128);
        CHECK(p.nblocks_n * 128 >= N && (p.nblocks_n - 1) * 128 < N && p.nblocks_n * 128 <= Npad, "gtt8_plan_narrow: N=%lld: %lld blocks", (long long)N, (long long)p.nblocks_n);
        CHECK(p.grid * 4 >= p.W * p.nblocks_n && (p.grid - 1) * 4 < p.W * p.nblocks_n, "gtt8_plan_narrow: Mpad=%lld N=%lld: grid", (long long)Mpad, (long long)N);
    }
    {
        const PrjPlan p = prj_plan(Mpad, Npad, gtt_target);
        check_chunks("prj_plan", Mpad, Npad, p.W, p.rows_per_wave, 128);
        check_ngroups("prj_plan", Mpad, Npad, p.ngroups, 64);
        CHECK(p.grid == p.ngroups * p.W, "prj_plan: Mpad=%lld Npad=%lld: grid", (long long)Mpad, (long long)Npad);
        CHECK(p.rows_per_wave <= ((int64_t)1 << 22), "prj_plan: Mpad=%lld Npad=%lld: %lld rows in one i32 accumulation", (long long)Mpad, (long long)Npad, (long long)p.rows_per_wave);
    }
}

// everything of a handle with M rows, N samples at sketch width L that is written into d_scratch64, d_part64, d_cpart, the candidates
static void audit_workspace(int L, int64_t M, int64_t N, int packed, int gq_target) {
    const int64_t Mpad = round_up(M, kGQRowsPerWave), Npad = round_up(N, packed ? 1024 : kSamplePad);
    const int64_t scratch = sum_scratch_capacity(kMaxSketchCols), LL = (int64_t)L * L;
    const int64_t part64 = part64_capacity(M, Mpad, N, Npad, L);
    // d_scratch64: the Gram of B = A Q (M rows) and the sample-side Grams (N rows); the eigen kernel / k_chol_inv folds the slices
    check_sum("d_scratch64 <- Gram of B (gram_num_parts(M))", L, "M", M, gram_num_parts(M), LL, scratch, true);
    check_sum("d_scratch64 <- sample-side Gram (gram_num_parts(N))", L, "N", N, gram_num_parts(N), LL, scratch, true);
    // c = b^T T: Omega's / launch_scale_rows' partials [omega_num_parts][L]; the exact path's [Mpad / 32][32] per 32-column block
    check_sum("d_scratch64 <- c of the sketch (omega_num_parts(Mpad))", L, "M", M, omega_num_parts(Mpad), L, scratch, false);
    check_sum("d_scratch64 <- c of a 32-column block (Mpad / 32 units)", L, "M", M, Mpad / 32, 32, scratch, false);
    // launch_post_k1: block hf of L / 32 writes post_k1_slices * 32 doubles at hf * kPostK1Scratch; launch_quantize_f32_cfold folds them
    const int s1 = post_k1_slices(Mpad / 32);
    CHECK((int64_t)s1 * 32 <= kPostK1Scratch, "launch_post_k1: L=%d M=%lld: %d slices x 32 > kPostK1Scratch", L, (long long)M, s1);
    CHECK((int64_t)(L / 32 - 1) * kPostK1Scratch + (int64_t)s1 * 32 <= scratch, "launch_post_k1: L=%d M=%lld: block %d ends past d_scratch64", L, (long long)M, L / 32 - 1);
    CHECK(s1 <= kSumSlicesMaxNarrow, "launch_quantize_f32_cfold: L=%d M=%lld: folds %d slices", L, (long long)M, s1);
    // d_part64: every writer
    CHECK(gram_num_parts(M) * LL <= part64, "d_part64 <- Gram of B: L=%d M=%lld N=%lld: %lld > %lld", L, (long long)M, (long long)N, (long long)(gram_num_parts(M) * LL), (long long)part64);
    CHECK(gram_num_parts(N) * LL <= part64, "d_part64 <- sample-side Gram: L=%d M=%lld N=%lld: %lld > %lld", L, (long long)M, (long long)N, (long long)(gram_num_parts(N) * LL), (long long)part64);
    CHECK(colsum_num_parts(Npad) * L <= part64 && 2 * tail_num_parts(Npad) * L <= part64 && absmax_num_parts(Mpad) * 32 <= part64,
          "d_part64 <- column sums / tail / abs-max: L=%d M=%lld N=%lld", L, (long long)M, (long long)N);
    // the Gram of the condensed features (gpca_rsvd_condensed: R <= M rows, L <= 64) lands in the same two buffers
    if (L <= 64) {
        const int64_t Rs[] = {M, M - 1, M / 2, 294912, 262144, 262145, 2097152};
        for (int64_t R : Rs) {
            if (R < 1 || R > M) continue;
            CHECK(gram_num_parts(R) * LL <= part64, "d_part64 <- Gram of R condensed features: L=%d M=%lld N=%lld R=%lld: %lld > %lld", L, (long long)M, (long long)N,
                  (long long)R, (long long)(gram_num_parts(R) * LL), (long long)part64);
            check_sum("d_scratch64 <- Gram of the condensed features", L, "R", R, gram_num_parts(R), LL, scratch, true);
        }
    }
    // gram_max_parts is what it says
    CHECK(gram_num_parts(M) <= gram_max_parts(M) && gram_num_parts(N) <= gram_max_parts(N), "gram_max_parts: M=%lld N=%lld", (long long)M, (long long)N);
    // launch_chol_inv_fold (L == 32, one workgroup folds P <= 64 parts): stage_orth takes it only behind `parts <= 64`, so the limit itself
    // is enforced by that branch; what is audited is the design's promise that the sample-side Gram up to 262 144 rows stays inside it
    if (N <= 262144) CHECK(gram_num_parts(N) <= 64, "launch_chol_inv_fold: N=%lld makes %lld parts", (long long)N, (long long)gram_num_parts(N));
    // gram blocks: rows per block a multiple of 32, every row in exactly one block
    for (int64_t rows : {M, N}) {
        const int64_t rpb = gram_rows_per_block(rows), P = gram_num_parts(rows);
        CHECK(rpb >= 32 && rpb % 32 == 0 && P * rpb >= rows && (P - 1) * rpb < rows, "gram blocks: rows=%lld rpb=%lld parts=%lld", (long long)rows, (long long)rpb, (long long)P);
    }
    // the tail of the orthonormalisation: k_quantize folds its partials itself only behind `tparts <= kFinishQFoldMax` (stage_orth: the limit
    // is enforced by that branch, launch_finish_q takes the rest); audited here: the tail's workgroups cover Npad exactly
    const int64_t tparts = tail_num_parts(Npad);
    CHECK(tparts * kTailRows >= Npad && (tparts - 1) * kTailRows < Npad, "tail_num_parts: Npad=%lld", (long long)Npad);
    // d_cpart
    const GqPlan gq = gq_plan(Mpad, gq_target);
    const int64_t cpart = cpart_capacity(gq.waves, Mpad, L);
    CHECK(gq.waves * L <= cpart && omega_num_parts(Mpad) * L <= cpart && (Mpad / 32) * 32 * (L / 32) <= cpart, "d_cpart: L=%d M=%lld", L, (long long)M);
    CHECK(omega_num_parts(Mpad) * 64 >= Mpad, "omega_num_parts: Mpad=%lld", (long long)Mpad);
    // scores candidates (L <= 64): one per workgroup and column; k_scores_sign holds kScoreParts x 64 of them in LDS
    const int64_t sp = scores_num_parts(N);
    CHECK(sp >= 1 && sp <= kScoreParts && sp * L <= scores_cand_capacity(), "scores candidates: L=%d N=%lld parts=%lld", L, (long long)N, (long long)sp);
    CHECK(colsum_num_parts(Npad) * kColsumRowsPerBlock >= Npad && absmax_num_parts(Mpad) * kAbsmaxRowsPerBlock >= Mpad, "colsum / absmax blocks");
}

// the workspace of gpca_project (Lp = round_up(k, 32) columns)
static void audit_project(int Lp, int64_t M, int packed) {
    const int64_t Mpad = round_up(M, kGQRowsPerWave);
    (void)packed;
    check_sum("project scratch <- c (omega_num_parts(Mpad))", Lp, "M", M, omega_num_parts(Mpad), Lp, project_scratch_capacity(Lp), false);
    CHECK(omega_num_parts(Mpad) * Lp <= project_cpart_capacity(Mpad, Lp), "project cpart: Lp=%d M=%lld", Lp, (long long)M);
    CHECK(absmax_num_parts(Mpad) * 32 <= project_part_capacity(Mpad, Lp) && 2 * (int64_t)Lp <= project_part_capacity(Mpad, Lp), "project part: Lp=%d M=%lld", Lp, (long long)M);
}

int main(int argc, char** argv) {
    const int nrand = argc > 1 ? std::atoi(argv[1]) : 300;
    const std::vector<int64_t> Ms = grid(100000000, nrand), Ns = grid(4194304, nrand);
    // a short list of the other axis for the two-dimensional checks (plans depend on both pads)
    const std::vector<int64_t> Nfew = {1, 255, 256, 257, 1023, 1025, 4096, 50000, 487409, 4194304};
    const std::vector<int64_t> Mfew = {1, 129, 4097, 100000, 1250000, 2097153, 10000000, 100000000};
    const int targets[][2] = {{1024, 2048}, {4, 4}, {256, 512}};
    for (int L : {32, 64, 128}) {
        for (int packed = 0; packed < 2; ++packed) {
            for (int64_t M : Ms) for (int64_t N : Nfew) audit_workspace(L, M, N, packed, 1024);
            for (int64_t N : Ns) for (int64_t M : Mfew) audit_workspace(L, M, N, packed, 1024);
            for (int64_t M : Ms) for (int Lp = 32; Lp <= L; Lp += 32) audit_project(Lp, M, packed);
        }
    }
    for (int packed = 0; packed < 2; ++packed)
        for (const auto& t : targets) {
            for (int64_t M : Ms) for (int64_t N : Nfew) audit_plans(M, N, packed, t[0], t[1]);
            for (int64_t N : Ns) for (int64_t M : Mfew) audit_plans(M, N, packed, t[0], t[1]);
        }
    std::printf("plan_audit: %ld checks, %ld failures (%zu row counts, %zu sample counts)\n", g_checks, g_fail, Ms.size(), Ns.size());
    return g_fail ? 1 : 0;
}
