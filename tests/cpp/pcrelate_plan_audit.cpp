// Extent audit of the PC-Relate host arithmetic (genomic_pca_amd/csrc/plan_math.h, the pcr_* functions): for kept-row counts, sample
// counts and coordinate counts at the tile edges and at their limits, every writer of pcrelate.hip stays inside the buffer
// gpca_pcrelate.cpp allocates for it, the stages and flush groups cover the kept rows once, and the staged reads stay inside a row's
// pitch.  Restates the kernels' index arithmetic on the host; includes the header the engine itself uses.  (The band -- entries,
// indices, tiles -- is audited with GRM's and KING's in band_plan_audit.cpp.)
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

// the kept-row axis: stages, flush groups, the grouped beta layout and the regression kernel's blocks
static void audit_rows(int64_t K, int P) {
    const int P1 = P + 1;
    const int64_t kpad = pcr_kpad(K), nst = pcr_stages(K), cap = pcr_beta_capacity(K, P);
    EXPECT(kpad >= K && kpad - K < kPcrBetaRows && kpad % kPcrBetaRows == 0, "kpad K=%lld", (long long)K);
    EXPECT(nst * kPcrStageRows >= K && (nst - 1) * kPcrStageRows < K, "stages K=%lld", (long long)K);
    // k_pcrelate reads the groups of 8 rows of every stage: the last one starts at (nst - 1) * 16 + 8
    const int64_t last_group = ((nst - 1) * kPcrStageRows + 8) >> 3;
    EXPECT((last_group + 1) * 8 * P1 <= cap, "k_pcrelate beta read K=%lld P=%d", (long long)K, P);
    // k_pcrelate_beta writes row kpad - 1, coefficient P
    const int64_t kr = kpad - 1;
    EXPECT(((kr >> 3) * P1 + P) * 8 + (kr & 7) < cap, "k_pcrelate_beta write K=%lld P=%d", (long long)K, P);
    EXPECT((K - 1) * P1 + P < cap, "row-major beta K=%lld P=%d", (long long)K, P);
    // flush groups: a whole number of stages, at most kPcrFlushRows rows, every stage in exactly one group
    const int64_t per = kPcrFlushRows / kPcrStageRows, ngroups = (nst + per - 1) / per;
    EXPECT(per * kPcrStageRows == kPcrFlushRows && kPcrFlushRows <= 256, "flush group");
    EXPECT(ngroups * per >= nst && (ngroups - 1) * per < nst, "flush groups K=%lld", (long long)K);
    // the hat matrix: coefficient j of wave j / width, slot j % width
    const int w = pcr_beta_width(P);
    EXPECT(w >= 1 && w * kPcrBetaWaves >= P1, "beta width P=%d", P);
    EXPECT(P / w < kPcrBetaWaves, "beta wave P=%d", P);
}

// the sample axis: design rows, invalid counts, the regression kernel's staged reads against the pitches of gpca_residency.cpp
static void audit_samples(int64_t N, int P) {
    const int64_t npad = pcr_npad(N);
    EXPECT(npad >= N && npad - N < kPcrTile, "npad N=%lld", (long long)N);
    const int64_t t1 = (N + kPcrTile - 1) / kPcrTile;
    EXPECT((t1 * kPcrTile - 1) * (P + 1) + P < pcr_x_capacity(N, P), "design row read N=%lld P=%d", (long long)N, P);
    EXPECT(t1 * kPcrTile - 1 < pcr_inv_capacity(N), "inv N=%lld", (long long)N);
    const int w = pcr_beta_width(P);
    EXPECT(((int64_t)(kPcrBetaWaves - 1) * N + (N - 1)) * w + (w - 1) < pcr_hat_capacity(N, P), "hat N=%lld P=%d", (long long)N, P);
    // int8 rows pad to kSamplePad samples, 2-bit rows to 1 024 samples (4 per byte); the regression kernel reads dwords of samples < N
    const int64_t ld8 = (N + kSamplePad - 1) / kSamplePad * kSamplePad, ld2 = (N + 1023) / 1024 * 1024 / 4;
    const int64_t last = (N - 1) / 4 * 4;
    EXPECT(last + 4 <= ld8 && last / 4 < ld2, "staged read past the pitch N=%lld", (long long)N);
}

int main() {
    static_assert(kPcrThreads == 4 * kPcrTile && kPcrStageRows == 16, "staging map: 2 sides x 128 samples x 2 row halves of 8");
    std::mt19937_64 rng(11);
    std::vector<int64_t> Ks = {1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193, 1000003, ((int64_t)1 << 31) - 1};
    std::vector<int64_t> Ns = {1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2085, 10000, 50000, 500000};
    for (int t = 0; t < 300; ++t) { Ks.push_back(1 + (int64_t)(rng() % 3000000)); Ns.push_back(1 + (int64_t)(rng() % 200000)); }
    for (int P = 0; P <= kPcrMaxPcs; ++P) {
        for (int64_t K : Ks) audit_rows(K, P);
        for (int64_t N : Ns) audit_samples(N, P);
    }
    printf("pcrelate_plan_audit: %lld checks, %lld failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
