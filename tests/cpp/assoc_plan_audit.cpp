// Extent audit of the association scan's host arithmetic (genomic_pca_amd/csrc/plan_math.h, the asc_* functions): for sample counts,
// column counts and bands at the tile edges and at their limits, every reader and writer of assoc.hip stays inside the buffer
// gpca_assoc.cpp allocates for it, the stages and flush groups cover the samples once, the workgroups cover the band's rows once, and
// the staged reads stay inside a row's pitch and inside the stage's LDS buffers.  Restates the kernels' index arithmetic on the host;
// includes the header the engine itself uses.
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

// the sample axis: stages, flush groups, the panel of B^T, the include words, the genotype reads against the pitches of
// gpca_residency.cpp
static void audit_samples(int64_t N, int L) {
    const int64_t npad = asc_npad(N), nst = asc_stages(N);
    const int lpad = asc_lpad(L);
    EXPECT(lpad >= L && (lpad == 32 || lpad == 64), "lpad L=%d", L);
    EXPECT(npad >= N && npad - N < kAscStage && npad == nst * kAscStage, "npad N=%lld", (long long)N);
    EXPECT(nst >= 1 && (nst - 1) * kAscStage < N, "stages N=%lld", (long long)N);
    // flush groups: a whole number of stages, at most kAscFlush samples, every stage in exactly one group
    const int64_t per = kAscFlush / kAscStage, ngroups = (nst + per - 1) / per;
    EXPECT(per * kAscStage == kAscFlush && kAscFlush <= 256, "flush group");
    EXPECT(ngroups * per >= nst && (ngroups - 1) * per < nst, "flush groups N=%lld", (long long)N);
    // asc_fetch_b: thread t, slot i reads 4 floats of column idx / 16 at sample n0 + 4 (idx % 16), idx = t + 256 i < 16 lpad
    const int64_t last_idx = (int64_t)kAscThreads * (2 * (lpad / 32)) - 1;
    EXPECT(last_idx / 16 == lpad - 1, "panel columns L=%d", L);
    EXPECT((last_idx / 16) * npad + (nst - 1) * kAscStage + 4 * (last_idx % 16) + 3 < asc_b_capacity(N, L), "panel read N=%lld L=%d", (long long)N, L);
    EXPECT((last_idx / 16) * kAscBPitch + 4 * (last_idx % 16) + 3 < (int64_t)lpad * kAscBPitch, "panel LDS write L=%d", L);
    // a lane reads 8 floats of column 32 j + c from sample 16 q + 8 h
    EXPECT((int64_t)(lpad - 1) * kAscBPitch + 16 * (kAscStage / 16 - 1) + 8 + 7 < (int64_t)lpad * kAscBPitch, "panel LDS read L=%d", L);
    EXPECT((kAscBPitch * 4) % 16 == 0 && kAscGPitch % 8 == 0, "LDS alignment");
    // the include words: two per stage
    EXPECT((nst - 1) * (kAscStage / 32) + 1 < asc_inc_capacity(N), "include words N=%lld", (long long)N);
    EXPECT(asc_inc_capacity(N) * 32 >= N, "include bits N=%lld", (long long)N);
    // the calls: thread t stages samples [32 (t % 2), + 32) of row t / 2; a lane reads 8 bytes of row 32 w + c from 16 q + 8 h
    EXPECT((kAscThreads / 2 - 1) * kAscGPitch + 32 + 31 < kAscRows * kAscGPitch, "calls LDS write");
    EXPECT((kAscRows - 1) * kAscGPitch + 16 * (kAscStage / 16 - 1) + 8 + 7 < kAscRows * kAscGPitch, "calls LDS read");
    // int8 rows pad to kSamplePad samples, 2-bit rows to 1 024 samples (4 per byte); the last read of a row ends at npad
    const int64_t ld8 = (N + kSamplePad - 1) / kSamplePad * kSamplePad, ld2 = (N + 1023) / 1024 * 1024 / 4;
    const int64_t ns = (nst - 1) * kAscStage + 32;
    EXPECT(ns + 32 <= ld8 && (ns >> 2) + 8 <= ld2, "staged read past the pitch N=%lld", (long long)N);
    EXPECT(ns % 16 == 0 && (ns >> 2) % 8 == 0 && ld8 % 16 == 0 && ld2 % 8 == 0, "staged read alignment N=%lld", (long long)N);
    // the per-row sums are 32-bit: gpca_assoc_linear refuses N >= 2^30
    EXPECT(N >= ((int64_t)1 << 30) || 4 * N < ((int64_t)1 << 32), "sums N=%lld", (long long)N);
}

// the band: workgroups cover its rows once; the last workgroup's writers stay inside xb, the sums, stats and rowinfo
static void audit_band(int64_t K, int64_t row0, int64_t row1, int T, int Pc) {
    const int L = T + Pc;
    const int64_t rows = row1 - row0, nb = asc_row_blocks(rows);
    EXPECT(row0 >= 0 && row1 <= K, "band in the kept rows");
    EXPECT(nb * kAscRows >= rows && (nb - 1) * kAscRows < rows, "row blocks rows=%lld", (long long)rows);
    // the last row a workgroup writes: kr < row1, so kr - row0 <= rows - 1, columns < L
    const int64_t last = rows - 1;
    EXPECT(last * L + (L - 1) < asc_xb_capacity(rows, L), "xb rows=%lld L=%d", (long long)rows, L);
    EXPECT(3 * last + 2 < asc_sums_capacity(rows), "sums rows=%lld", (long long)rows);
    EXPECT((last * T + (T - 1)) * 3 + 2 < asc_stats_capacity(rows, T), "stats rows=%lld T=%d", (long long)rows, T);
    EXPECT(4 * last + 3 < asc_info_capacity(rows), "rowinfo rows=%lld", (long long)rows);
    // a row of the band belongs to exactly one workgroup and one wave slot
    for (int64_t a : {row0, (row0 + row1) / 2, row1 - 1}) {
        const int64_t blk = (a - row0) / kAscRows, r = (a - row0) % kAscRows;
        EXPECT(blk < nb && r / 32 < kAscThreads / 64, "row %lld in no workgroup", (long long)a);
    }
}

int main() {
    static_assert(kAscThreads == 2 * kAscRows && kAscStage == 64 && kAscMaxCols == 64, "staging map: 2 threads x 32 samples per row");
    std::mt19937_64 rng(12);
    std::vector<int64_t> Ks = {1, 2, 31, 32, 33, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 8193, 1000003, ((int64_t)1 << 31) - 1};
    std::vector<int64_t> Ns = {1, 2, 3, 4, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2085, 10000, 50000, 500000,
                               ((int64_t)1 << 30) - 1};
    for (int t = 0; t < 300; ++t) { Ks.push_back(1 + (int64_t)(rng() % 3000000)); Ns.push_back(1 + (int64_t)(rng() % 200000)); }
    for (int L = 1; L <= kAscMaxCols; ++L)
        for (int64_t N : Ns) audit_samples(N, L);
    for (int64_t K : Ks)
        for (int t = 0; t < 24; ++t) {
            const int T = 1 + (int)(rng() % 64), Pc = (int)(rng() % (uint64_t)(65 - T));
            int64_t r0 = t == 0 ? 0 : (int64_t)(rng() % (uint64_t)K), r1 = t == 0 ? K : r0 + 1 + (int64_t)(rng() % (uint64_t)(K - r0));
            for (int64_t e0 : {r0, r0 / kAscRows * kAscRows}) audit_band(K, e0, r1, T, Pc);
            audit_band(K, r0, r0 + 1, T, Pc);
        }
    printf("assoc_plan_audit: %lld checks, %lld failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
