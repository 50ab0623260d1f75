// Extent audit of the logistic score scan's host arithmetic (genomic_pca_amd/csrc/plan_math.h, the asr_* functions beside the asc_*
// ones the scan shares with k_assoc): for sample counts, trait and covariate counts and bands at the tile edges and at their limits,
// every reader and writer of assoc_score.hip stays inside the buffer gpca_assoc_score.cpp allocates for it, the panel's columns are
// laid out once and inside the padded panel with every w column in the first block of 32, the count kernel's chunks cover the samples
// once and its reads stay inside a row's pitch, and the workgroups of the three kernels cover the band's rows once.  Restates the
// kernels' index arithmetic on the host; includes the header the engine itself uses.
#include "plan_math.h"

#include <cstdio>
#include <random>
#include <vector>

using namespace gpca;

static long long g_checks = 0, g_fail = 0;
#define EXPECT(cond, ...)                                                        \
    do {                                                                         \
        ++g_checks;                                                              \
        if (!(cond)) { if (++g_fail <= 20) { printf("FAIL " __VA_ARGS__); printf("\n"); } } \
    } while (0)

// the panel: T (Pc + 3) = L columns, each index used once, w in the first block
static void audit_columns(int T, int Pc) {
    const int L = asr_cols(T, Pc), lpad = asc_lpad(L);
    EXPECT(L >= 3 && L <= kAsrMaxCols && lpad >= L, "L T=%d Pc=%d", T, Pc);
    EXPECT(T <= asr_max_traits(Pc) && (asr_max_traits(Pc) + 1) * (Pc + 3) > kAsrMaxCols, "max traits Pc=%d", Pc);
    std::vector<int> used((size_t)L, 0);
    for (int t = 0; t < T; ++t) {
        EXPECT(asr_col_w(t) < 32 && asr_col_w(t) < L, "w column T=%d", T);
        const int cw = asr_col_w(t), cr = asr_col_r(T, t);
        EXPECT(cw >= 0 && cw < L && cr >= 0 && cr < L, "w, r columns T=%d Pc=%d", T, Pc);
        if (cw >= 0 && cw < L) used[(size_t)cw]++;
        if (cr >= 0 && cr < L) used[(size_t)cr]++;
        for (int j = 0; j <= Pc; ++j) {
            const int ca = asr_col_a(T, Pc, t, j);
            EXPECT(ca >= 0 && ca < L, "A column T=%d Pc=%d", T, Pc);
            if (ca >= 0 && ca < L) used[(size_t)ca]++;
        }
    }
    for (int c = 0; c < L; ++c) EXPECT(used[(size_t)c] == 1, "column %d used %d times T=%d Pc=%d", c, used[(size_t)c], T, Pc);
}

// the sample axis for a panel of L columns: the stages and the panel are k_assoc's (audited in assoc_plan_audit.cpp; the reads that
// depend on L are restated), the count kernel's chunks are this scan's own
static void audit_samples(int64_t N, int L) {
    const int64_t npad = asc_npad(N), nst = asc_stages(N);
    const int lpad = asc_lpad(L);
    EXPECT(npad >= N && npad - N < kAscStage && npad == nst * kAscStage, "npad N=%lld", (long long)N);
    // asc_fetch_b / asc_put_b with NB = lpad / 32
    const int64_t last_idx = (int64_t)kAscThreads * (2 * (lpad / 32)) - 1;
    EXPECT(last_idx / 16 == lpad - 1, "panel columns L=%d", L);
    EXPECT((last_idx / 16) * npad + (nst - 1) * kAscStage + 4 * (last_idx % 16) + 3 < asc_b_capacity(N, L), "panel read N=%lld L=%d", (long long)N, L);
    EXPECT((last_idx / 16) * kAscBPitch + 4 * (last_idx % 16) + 3 < (int64_t)lpad * kAscBPitch, "panel LDS write L=%d", L);
    EXPECT((int64_t)(lpad - 1) * kAscBPitch + 16 * (kAscStage / 16 - 1) + 8 + 7 < (int64_t)lpad * kAscBPitch, "panel LDS read L=%d", L);
    // the q product reads block 0 only: columns 0 .. 31 of the staged panel
    EXPECT((int64_t)31 * kAscBPitch + 16 * (kAscStage / 16 - 1) + 8 + 7 < (int64_t)lpad * kAscBPitch, "q LDS read L=%d", L);
    // the calls of a stage
    EXPECT((kAscThreads / 2 - 1) * kAscGPitch + 32 + 31 < kAscRows * kAscGPitch, "calls LDS write");
    EXPECT((nst - 1) * (kAscStage / 32) + 1 < asc_inc_capacity(N), "include words N=%lld", (long long)N);
    // k_assoc_score_count: lane l of a row's wave reads 32 samples at n0 = 32 l + kAsrChunk c for every n0 < npad: each 32-sample
    // word below npad is read once, the include word exists, and the read ends inside the row's pitch with its alignment
    const int64_t chunks = asr_count_chunks(N);
    EXPECT(chunks * kAsrChunk >= npad && (chunks - 1) * kAsrChunk < npad, "count chunks N=%lld", (long long)N);
    EXPECT(kAsrChunk == 64 * 32 && kAsrCountThreads == 64 * kAsrCountRows, "count kernel: a wave per row, 32 samples per lane");
    const int64_t n0_last = npad - 32;                         // the largest n0 below npad (npad is a multiple of 64)
    EXPECT(n0_last % 32 == 0 && (n0_last >> 5) < asc_inc_capacity(N), "count include word N=%lld", (long long)N);
    const int64_t ld8 = (N + kSamplePad - 1) / kSamplePad * kSamplePad, ld2 = (N + 1023) / 1024 * 1024 / 4;
    EXPECT(n0_last + 32 <= ld8 && (n0_last >> 2) + 8 <= ld2, "count read past the pitch N=%lld", (long long)N);
    EXPECT(n0_last % 16 == 0 && (n0_last >> 2) % 8 == 0, "count read alignment N=%lld", (long long)N);
    EXPECT(N >= ((int64_t)1 << 30) || 4 * N < ((int64_t)1 << 32), "sums N=%lld", (long long)N);
}

// the band: the workgroups of the three kernels cover its rows once; the last writers stay inside dv, the sums, stats, ua and rowinfo
static void audit_band(int64_t K, int64_t row0, int64_t row1, int T, int Pc) {
    const int L = asr_cols(T, Pc);
    const int64_t rows = row1 - row0, nb = asc_row_blocks(rows), nc = asr_count_blocks(rows);
    EXPECT(row0 >= 0 && row1 <= K, "band in the kept rows");
    EXPECT(nb * kAscRows >= rows && (nb - 1) * kAscRows < rows, "row blocks rows=%lld", (long long)rows);
    EXPECT(nc * kAsrCountRows >= rows && (nc - 1) * kAsrCountRows < rows, "count blocks rows=%lld", (long long)rows);
    EXPECT(nc >= nb && (K >= ((int64_t)1 << 31) || nc < ((int64_t)1 << 31)), "grids rows=%lld", (long long)rows);
    const int64_t last = rows - 1;
    EXPECT(last * L + (L - 1) < asr_dv_capacity(rows, L), "dv rows=%lld L=%d", (long long)rows, L);
    EXPECT(3 * last + 2 < asr_sums_capacity(rows), "sums rows=%lld", (long long)rows);
    EXPECT((last * T + (T - 1)) * 5 + 4 < asr_stats_capacity(rows, T), "stats rows=%lld T=%d", (long long)rows, T);
    EXPECT((last * T + (T - 1)) * (Pc + 3) + (Pc + 2) < asr_ua_capacity(rows, T, Pc), "ua rows=%lld T=%d Pc=%d", (long long)rows, T, Pc);
    EXPECT(asr_ua_capacity(rows, T, Pc) == asr_dv_capacity(rows, L), "ua and dv hold the same values");
    EXPECT(5 * last + 4 < asr_info_capacity(rows), "rowinfo rows=%lld", (long long)rows);
    // the finish kernel reads dv columns through asr_col_*: inside the row (audit_columns) and the row inside dv
    EXPECT(last * L + asr_col_a(T, Pc, T - 1, Pc) < asr_dv_capacity(rows, L), "finish read rows=%lld", (long long)rows);
    for (int64_t a : {row0, (row0 + row1) / 2, row1 - 1}) {
        const int64_t blk = (a - row0) / kAscRows, r = (a - row0) % kAscRows;
        EXPECT(blk < nb && r / 32 < kAscThreads / 64, "row %lld in no workgroup", (long long)a);
        EXPECT((a - row0) / kAsrCountRows < nc && (a - row0) % kAsrCountRows < kAsrCountThreads / 64, "row %lld in no count wave", (long long)a);
    }
}

int main() {
    static_assert(kAscThreads == 2 * kAscRows && kAscStage == 64 && kAsrMaxCols == 64, "staging map: 2 threads x 32 samples per row");
    std::mt19937_64 rng(13);
    std::vector<int64_t> Ks = {1, 2, 3, 4, 5, 31, 32, 33, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 8193, 1000003, ((int64_t)1 << 31) - 1};
    std::vector<int64_t> Ns = {1, 2, 3, 4, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 2085, 4096, 4097,
                               10000, 50000, 500000, ((int64_t)1 << 30) - 1};
    for (int t = 0; t < 300; ++t) { Ks.push_back(1 + (int64_t)(rng() % 3000000)); Ns.push_back(1 + (int64_t)(rng() % 200000)); }
    // every (T, Pc) the call accepts, hence every L it can reach from 3 to 64
    std::vector<int> seenL(kAsrMaxCols + 1, 0);
    for (int Pc = 0; Pc + 3 <= kAsrMaxCols; ++Pc)
        for (int T = 1; T <= asr_max_traits(Pc); ++T) { audit_columns(T, Pc); seenL[(size_t)asr_cols(T, Pc)] = 1; }
    for (int L = 3; L <= kAsrMaxCols; ++L) {
        EXPECT(seenL[(size_t)L] == 1, "no (T, Pc) gives L=%d", L);
        for (int64_t N : Ns) audit_samples(N, L);
    }
    for (int64_t K : Ks)
        for (int t = 0; t < 24; ++t) {
            const int Pc = (int)(rng() % 62), T = 1 + (int)(rng() % (uint64_t)asr_max_traits(Pc));
            int64_t r0 = t == 0 ? 0 : (int64_t)(rng() % (uint64_t)K), r1 = t == 0 ? K : r0 + 1 + (int64_t)(rng() % (uint64_t)(K - r0));
            for (int64_t e0 : {r0, r0 / kAscRows * kAscRows}) audit_band(K, e0, r1, T, Pc);
            audit_band(K, r0, r0 + 1, T, Pc);
        }
    printf("assoc_score_plan_audit: %lld checks, %lld failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
