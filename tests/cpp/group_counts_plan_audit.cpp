// Extent audit of the per-group genotype counts' host arithmetic (genomic_pca_amd/csrc/plan_math.h, the gc_* functions): walks, thread by
// thread and stage by stage, every staged read of a row and of the one-hot matrix (group_counts.hip) and holds it inside the row's pitch
// (gpca_residency.cpp) or the buffer gpca_group_counts.cpp allocates, with its alignment; walks every (workgroup, wave, lane, register,
// column block) of a band and counts the writers of every counts entry (exactly one); sums the allocations against the GPCA_ERR_OOM sum;
// and bounds the i32 accumulators.  Restates the kernels' index arithmetic on the host; includes the header the engine itself uses.
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

// C/D of a 32 x 32 MFMA (kernels.h: acc_row)
static int acc_row(int row0, int e, int h) { return row0 + (e & 3) + 8 * (e >> 2) + 4 * h; }

// the sample axis: every thread's reads of every stage (all stages up to `full_stages`, then the first and the last ones)
static void audit_samples(int64_t N, int P, int64_t full_stages) {
    const int64_t npad = gc_npad(N), nst = gc_stages(N);
    const int ppad = gc_ppad(P), nb = ppad / 32;
    EXPECT(ppad >= P && (ppad == 32 || ppad == 64) && ppad <= kGcMaxGroups, "ppad P=%d", P);
    EXPECT(npad >= N && npad - N < kGcStage && npad == nst * kGcStage && nst >= 1, "npad N=%lld", (long long)N);
    // int8 rows pad to kSamplePad samples, 2-bit rows to 1 024 samples (4 per byte); the pitch is at least that
    const int64_t ld8 = (N + kSamplePad - 1) / kSamplePad * kSamplePad, ld2 = (N + 1023) / 1024 * 1024 / 4;
    const int64_t ocap = gc_onehot_capacity(N, P);
    EXPECT(ld8 % 16 == 0 && ld2 % 8 == 0 && npad % 16 == 0 && kGcPitch % 16 == 0, "alignment N=%lld", (long long)N);
    for (int64_t s = 0; s < nst; ++s) {
        if (s >= full_stages && s + full_stages < nst) { s = nst - full_stages - 1; continue; }
        for (int t = 0; t < kGcThreads; ++t) {
            // the calls: 32 bytes (int8) or 8 bytes (2-bit) of row t / 2
            const int64_t o8 = gc_row_offset(false, t, s), o2 = gc_row_offset(true, t, s);
            EXPECT(o8 >= 0 && o8 + 32 <= ld8 && o8 % 16 == 0, "int8 read N=%lld s=%lld t=%d", (long long)N, (long long)s, t);
            EXPECT(o2 >= 0 && o2 + 8 <= ld2 && o2 % 8 == 0, "2-bit read N=%lld s=%lld t=%d", (long long)N, (long long)s, t);
            // ... written to LDS at (t / 2) pitch + 32 (t % 2), 32 bytes
            EXPECT((t >> 1) * kGcPitch + 32 * (t & 1) + 32 <= kGcRows * kGcPitch, "calls LDS write t=%d", t);
            // the one-hot matrix: threads below 4 x 32 nb read 16 bytes of column t / 4
            if ((t >> 2) < 32 * nb) {
                const int64_t oo = gc_onehot_offset(npad, t, s);
                EXPECT(oo >= 0 && oo + 16 <= ocap && oo % 16 == 0, "one-hot read N=%lld P=%d s=%lld t=%d", (long long)N, P, (long long)s, t);
                EXPECT((t >> 2) < ppad && oo / npad == (t >> 2) && (oo + 15) / npad == (t >> 2), "one-hot read leaves its column t=%d", t);
                EXPECT((t >> 2) * kGcPitch + 16 * (t & 3) + 16 <= 32 * nb * kGcPitch, "one-hot LDS write t=%d", t);
            }
        }
    }
    // every one-hot byte of a stage is staged exactly once
    std::vector<int> seen((size_t)ppad * kGcStage, 0);
    for (int t = 0; t < kGcThreads; ++t)
        if ((t >> 2) < 32 * nb)
            for (int b = 0; b < 16; ++b) seen[(size_t)(t >> 2) * kGcStage + 16 * (t & 3) + b]++;
    bool once = true;
    for (int v : seen) once = once && v == 1;
    EXPECT(once, "one-hot stage covered once P=%d", P);
    // the LDS reads of a lane: 16 bytes of row 32 w + c (or column 32 j + c) at block q, half h
    for (int w = 0; w < kGcThreads / 64; ++w)
        for (int c = 0; c < 32; ++c)
            for (int h = 0; h < 2; ++h)
                for (int q = 0; q < kGcStage / kGcBlock; ++q) {
                    const int a = (32 * w + c) * kGcPitch + 16 * h + kGcBlock * q;
                    EXPECT(a % 16 == 0 && a + 16 <= kGcRows * kGcPitch && a % kGcPitch + 16 <= kGcStage, "calls LDS read");
                    for (int j = 0; j < nb; ++j) {
                        const int b = (32 * j + c) * kGcPitch + 16 * h + kGcBlock * q;
                        EXPECT(b % 16 == 0 && b + 16 <= 32 * nb * kGcPitch && b % kGcPitch + 16 <= kGcStage, "one-hot LDS read");
                    }
                }
    // the one-hot kernel: thread q of column p writes the dword q < npad / 4
    EXPECT((int64_t)(ppad - 1) * npad + 4 * (npad / 4 - 1) + 4 <= ocap && npad % 4 == 0, "one-hot write N=%lld P=%d", (long long)N, P);
    // the accumulators: a count is at most N, and gpca_group_counts refuses N >= 2^30
    EXPECT(N < ((int64_t)1 << 30) && N <= ((int64_t)1 << 31) - 1, "i32 accumulators N=%lld", (long long)N);
    // the OOM sum is the allocations: one-hot bytes, labels (i32), sizes (u32), counts (u32), the invalid-genotype word
    for (int64_t rows : {(int64_t)1, (int64_t)129, (int64_t)1000003}) {
        const double sum = (double)ocap * 1.0 + (double)gc_label_capacity(N) * 4.0 + (double)gc_size_capacity() * 4.0 +
                           (double)gc_counts_capacity(rows, P) * 4.0 + 8.0;
        EXPECT(sum == gc_call_bytes(N, rows, P), "OOM sum N=%lld rows=%lld P=%d", (long long)N, (long long)rows, P);
    }
    EXPECT(gc_size_capacity() >= P && gc_label_capacity(N) >= N, "sizes and labels");
}

// the band: every counts entry has exactly one writer, inside the buffer
static void audit_band(int64_t row0, int64_t row1, int P) {
    const int64_t rows = row1 - row0, nblk = gc_row_blocks(rows), cap = gc_counts_capacity(rows, P);
    const int nb = gc_ppad(P) / 32;
    EXPECT(nblk * kGcRows >= rows && (nblk - 1) * kGcRows < rows, "row blocks rows=%lld", (long long)rows);
    std::vector<uint8_t> hits((size_t)cap, 0);
    bool inside = true;
    for (int64_t blk = 0; blk < nblk; ++blk)
        for (int w = 0; w < kGcThreads / 64; ++w)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < nb; ++j) {
                    const int c = lane & 31, h = lane >> 5, p = 32 * j + c;
                    if (p >= P) continue;
                    for (int e = 0; e < 16; ++e) {
                        const int64_t kr = row0 + blk * kGcRows + acc_row(32 * w, e, h);
                        if (kr >= row1) continue;
                        for (int k = 0; k < 3; ++k) {
                            const int64_t ix = gc_counts_index(kr - row0, P, p, k);
                            if (ix < 0 || ix >= cap) { inside = false; continue; }
                            if (hits[(size_t)ix] < 255) hits[(size_t)ix]++;
                        }
                    }
                }
    EXPECT(inside, "a counts write leaves the buffer rows=%lld P=%d", (long long)rows, P);
    bool once = true;
    for (uint8_t v : hits) once = once && v == 1;
    EXPECT(once, "every counts entry written exactly once row0=%lld rows=%lld P=%d", (long long)row0, (long long)rows, P);
}

int main() {
    static_assert(kGcThreads == 2 * kGcRows && kGcStage == 64 && kGcBlock == 32 && kGcMaxGroups == 64, "staging map: 2 threads x 32 samples per row");
    std::mt19937_64 rng(17);
    std::vector<int64_t> Ns = {1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2085, 10000, 50000,
                               500000, ((int64_t)1 << 30) - 1};
    for (int t = 0; t < 60; ++t) Ns.push_back(1 + (int64_t)(rng() % 200000));
    for (int P = 1; P <= kGcMaxGroups; ++P)
        for (int64_t N : Ns) audit_samples(N, P, N <= 4096 ? ((int64_t)1 << 40) : 3);
    std::vector<int64_t> Rs = {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 385, 1000};
    for (int P = 1; P <= kGcMaxGroups; ++P)
        for (int64_t r : Rs)
            for (int64_t r0 : {(int64_t)0, (int64_t)5, (int64_t)128}) audit_band(r0, r0 + r, P);
    printf("group_counts_plan_audit: %lld checks, %lld failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
