// Extent audit of the windowed-LD host arithmetic (genomic_pca_amd/csrc/plan_math.h, the ld_* functions): for band sizes, window widths and
// sample counts at the tile edges and at their limits, every writer of ld.hip stays inside the buffer gpca_ld.cpp allocates for it, the
// grid covers every slot of the band exactly once, and the staged reads stay inside a row's pitch.  Restates the kernels' index
// arithmetic on the host; includes the header the engine itself uses.  With arguments `rows weff N` (any number of triples) it prints
// the launch plan of each triple instead (tests/test_gpu_ld_exact.py holds its Python mirror of the plan to these lines).
#include "plan_math.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace gpca;

static long long g_checks = 0, g_fail = 0;
#define EXPECT(cond, ...)                                                        \
    do {                                                                         \
        ++g_checks;                                                              \
        if (!(cond)) { if (++g_fail <= 20) { printf("FAIL " __VA_ARGS__); printf("\n"); } } \
    } while (0)

// the last slot index a row block / chunk / wave tile of k_ld can store to, against the plane capacity; and tile coverage of the band
static void audit_band(int64_t K, int64_t row0, int64_t rows, int64_t wmax, int64_t weff) {
    const int64_t row1 = row0 + rows;
    const int64_t plane = rows * wmax, cap = ld_ws_capacity(rows, wmax);
    EXPECT(cap == kLdProducts * plane, "ws capacity rows=%lld wmax=%lld", (long long)rows, (long long)wmax);
    const int64_t nrb = ld_row_blocks(rows), nch = ld_col_chunks(weff);
    EXPECT(nrb * kLdRows >= rows && (nrb - 1) * kLdRows < rows, "row blocks rows=%lld", (long long)rows);
    // k_ld: the largest (i, j) pair any active tile holds, clipped as the epilogue clips it (i < row1, i < j <= i + weff, j < K)
    const int64_t i_max = row1 - 1, j_max = std::min(K - 1, i_max + weff);
    if (j_max > i_max) {
        const int64_t ix = (i_max - row0) * wmax + (j_max - i_max - 1);
        EXPECT(ix < plane && (kLdProducts - 1) * plane + ix < cap, "k_ld store rows=%lld wmax=%lld weff=%lld", (long long)rows, (long long)wmax, (long long)weff);
    }
    // coverage: for the first and last row of every row block (and a middle one), every in-window column lies in an active tile
    for (int64_t rb = 0; rb < nrb; rb += std::max<int64_t>(1, nrb / 7)) {
        const int64_t i0 = row0 + rb * kLdRows;
        for (int64_t i : {i0, i0 + 31, i0 + 32, i0 + kLdRows - 1}) {
            if (i >= row1) continue;
            for (int64_t j : {i + 1, i + weff / 2 + 1, i + weff}) {
                if (j <= i || j >= K || j > i + weff) continue;
                const int64_t T = (j - i0) / 32, rt = (i - i0) / 32, chunk = T / (kLdCols / 32);
                EXPECT(chunk < nch, "chunk of column %lld beyond the grid (weff=%lld)", (long long)(j - i0), (long long)weff);
                EXPECT(T >= rt && 32 * (T - rt) < weff + 32, "tile (%lld, %lld) holds an in-window pair but is skipped (weff=%lld)", (long long)rt, (long long)T, (long long)weff);
            }
        }
    }
    // k_ld_finish: r2 / counts / above
    const int64_t nwords = ld_above_words(wmax), nwb = (nwords + 3) / 4;
    EXPECT(nwords * 64 >= wmax && (nwords - 1) * 64 < wmax, "above words wmax=%lld", (long long)wmax);
    const int64_t t = rows - 1, d = wmax - 1;
    EXPECT(t * wmax + d < ld_r2_capacity(rows, wmax), "r2 rows=%lld wmax=%lld", (long long)rows, (long long)wmax);
    EXPECT(6 * (t * wmax + d) + 5 < ld_counts_capacity(rows, wmax), "counts rows=%lld wmax=%lld", (long long)rows, (long long)wmax);
    EXPECT(t * nwords + (nwords - 1) < ld_above_capacity(rows, wmax), "above rows=%lld wmax=%lld", (long long)rows, (long long)wmax);
    EXPECT(nwb * 4 >= nwords, "finish grid wmax=%lld", (long long)wmax);
    // k_ld_vec: rows [row0, hi), hi = the furthest window end
    const int64_t hi = std::max(row1, std::min(K, row1 - 1 + weff + 1));
    EXPECT(3 * (hi - 1 - row0) + 2 < ld_stat_capacity(row0, hi), "stat row0=%lld hi=%lld", (long long)row0, (long long)hi);
    EXPECT(j_max <= i_max || 3 * (j_max - row0) + 2 < ld_stat_capacity(row0, hi), "stat read of column %lld", (long long)j_max);
}

// the sample axis: stages cover [0, N) once, the splits cover the stages once, and a staged 16-sample read stays inside the row pitch
static void audit_samples(int64_t N, int64_t nblocks) {
    const int64_t nst = ld_stages(N);
    EXPECT(nst * kLdStage >= N && (nst - 1) * kLdStage < N, "stages N=%lld", (long long)N);
    const int64_t per = ld_stages_per_split(nblocks, nst), S = ld_splits(nblocks, nst);
    EXPECT(per >= 1 && S >= 1 && S * per >= nst && (S - 1) * per < nst, "splits N=%lld nblocks=%lld per=%lld S=%lld", (long long)N, (long long)nblocks, (long long)per, (long long)S);
    EXPECT(S <= 65535, "grid.y N=%lld nblocks=%lld S=%lld", (long long)N, (long long)nblocks, (long long)S);
    // pitches of gpca_residency.cpp: int8 rows pad to kSamplePad samples, 2-bit rows to 1 024 samples (4 per byte)
    const int64_t ld8 = (N + kSamplePad - 1) / kSamplePad * kSamplePad, ld2 = (N + 1023) / 1024 * 1024 / 4;
    EXPECT(nst * kLdStage <= ld8, "int8 stage read past the pitch N=%lld", (long long)N);
    EXPECT(nst * kLdStage / 4 <= ld2, "2-bit stage read past the pitch N=%lld", (long long)N);
    EXPECT((N + 15) / 16 * 16 <= ld8 && (N + 15) / 16 * 4 <= ld2, "k_ld_vec read past the pitch N=%lld", (long long)N);
}

// print mode: the launch plan of k_ld for each (rows, weff, N) triple of the command line, one line per triple, from the header's own
// functions: workgroups, column chunks, sample stages, stages per split, splits, and whether the sums meet in plain stores or atomics
static int print_plans(int argc, char** argv) {
    if ((argc - 1) % 3 != 0) { fprintf(stderr, "usage: ld_plan_audit [rows weff N]...\n"); return 2; }
    for (int a = 1; a + 2 < argc; a += 3) {
        const int64_t rows = atoll(argv[a]), weff = atoll(argv[a + 1]), N = atoll(argv[a + 2]);
        const int64_t nch = ld_col_chunks(weff), nb = ld_row_blocks(rows) * nch, nst = ld_stages(N);
        const int64_t per = ld_stages_per_split(nb, nst), S = ld_splits(nb, nst);
        printf("%lld %lld %lld: %lld %lld %lld %lld %lld %s\n", (long long)rows, (long long)weff, (long long)N, (long long)nb, (long long)nch,
               (long long)nst, (long long)per, (long long)S, S > 1 ? "atomic" : "plain");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) return print_plans(argc, argv);
    static_assert(kLdRows * (kLdStage / 16) % kLdThreads == 0 && (kLdRows + kLdCols) * (kLdStage / 16) % kLdThreads == 0, "staging map covers the stage");
    static_assert(kLdCols / 32 == kLdThreads / 64, "one column tile per wave");
    std::mt19937_64 rng(7);
    std::vector<int64_t> Rs = {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 4096, 1000003, ((int64_t)1 << 31) - 1};
    std::vector<int64_t> Ws = {1, 2, 31, 32, 33, 49, 50, 63, 64, 65, 95, 96, 97, 127, 128, 129, 200, 1000, 4097, 1 << 20, ((int64_t)1 << 31) - 1};
    std::vector<int64_t> Ns = {1, 2, 15, 16, 17, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2085, 10000, 40000, 500000, ((int64_t)1 << 29) - 1};
    for (int t = 0; t < 300; ++t) {
        Rs.push_back(1 + (int64_t)(rng() % 3000000)); Ws.push_back(1 + (int64_t)(rng() % 100000)); Ns.push_back(1 + (int64_t)(rng() % 4194304));
    }
    for (int64_t rows : Rs)
        for (int64_t wmax : Ws) {
            if ((double)rows * (double)wmax * 6.0 > 9.0e18) continue;       // (the preflight refuses such a band long before)
            for (int64_t weff : {(int64_t)1, wmax / 2, wmax}) {
                if (weff < 1) continue;
                for (int64_t row0 : {(int64_t)0, (int64_t)77}) {
                    audit_band(row0 + rows + weff + 5, row0, rows, wmax, weff);      // windows never reach K
                    audit_band(row0 + rows, row0, rows, wmax, weff);                 // the band ends at K
                }
            }
        }
    for (int64_t N : Ns)
        for (int64_t nb : {(int64_t)1, (int64_t)2, (int64_t)7, (int64_t)100, (int64_t)1023, (int64_t)1024, (int64_t)50000}) audit_samples(N, nb);
    printf("ld_plan_audit: %lld checks, %lld failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
