// Extent audit of the f2 jackknife blocks' host arithmetic (genomic_pca_amd/csrc/plan_math.h, the fb_* functions): the pair map is a
// bijection onto 0 .. pairs - 1 for every P, and every pair has exactly one (thread, slot) owner; walks, workgroup by workgroup and
// tile by tile, every staged read of the counts workspace, every LDS write and read (f2_blocks.hip) and every (block, pair) the flush
// can address, and holds them inside the buffers gpca_f2_blocks.cpp allocates; sums the allocations against the GPCA_ERR_OOM sum; and
// bounds the i64 sums and i32 counts of a call.  Restates the kernel's index arithmetic on the host; includes the header the engine
// itself uses.
#include "plan_math.h"

#include <cmath>
#include <cstdio>
#include <vector>

using namespace gpca;

static long long g_checks = 0, g_fail = 0;
#define EXPECT(cond, ...)                                                        \
    do {                                                                         \
        ++g_checks;                                                              \
        if (!(cond)) { if (++g_fail <= 20) { printf("FAIL " __VA_ARGS__); printf("\n"); } } \
    } while (0)

// the pair map and the owners of the pairs
static void audit_pairs(int P) {
    const int pairs = fb_pairs(P), slots = fb_slots(P);
    EXPECT(pairs == P * (P - 1) / 2 && slots >= 1 && slots <= kFbSlots && slots * kFbThreads >= pairs && (slots - 1) * kFbThreads < pairs, "slots P=%d", P);
    // the launcher rounds the slots up to 1, 2, 4 or 8
    const int launched = slots <= 1 ? 1 : slots <= 2 ? 2 : slots <= 4 ? 4 : 8;
    EXPECT(launched >= slots && launched <= kFbSlots, "launched slots P=%d", P);
    std::vector<int> seen((size_t)pairs, 0), owner((size_t)pairs, 0);
    for (int i = 1; i < P; ++i)
        for (int j = 0; j < i; ++j) {
            const int q = fb_pair_index(i, j);
            EXPECT(q >= 0 && q < pairs, "pair index P=%d i=%d j=%d", P, i, j);
            if (q < 0 || q >= pairs) continue;
            seen[(size_t)q]++;
            EXPECT(fb_pair_i(q) == i && fb_pair_j(q) == j, "pair map inverse P=%d q=%d", P, q);
            EXPECT(i < kFbPitch && j < kFbPitch && i < 64 && j < 64, "a pair's groups index the LDS row and the 64-bit mask P=%d", P);
        }
    for (int t = 0; t < kFbThreads; ++t)
        for (int s = 0; s < launched; ++s) {
            const int q = t + kFbThreads * s;
            if (q < pairs) owner[(size_t)q]++;
        }
    bool bij = true, once = true;
    for (int q = 0; q < pairs; ++q) { bij = bij && seen[(size_t)q] == 1; once = once && owner[(size_t)q] == 1; }
    EXPECT(bij, "the pair map is a bijection P=%d", P);
    EXPECT(once, "every pair has one owner P=%d", P);
}

// every read of the counts workspace, every LDS access and every output index of a call
static void audit_rows(int64_t rows, int P, int64_t B) {
    const int64_t nblk = fb_row_blocks(rows), ccap = gc_counts_capacity(rows, P), bcap = fb_block_capacity(rows), ocap = fb_out_capacity(B, P);
    EXPECT(nblk * kFbRun >= rows && (nblk - 1) * kFbRun < rows && nblk < ((int64_t)1 << 31), "row blocks rows=%lld", (long long)rows);
    EXPECT(fb_lds_bytes() <= 64 * 1024 && fb_lds_bytes() == 2 * 8 * kFbTile * kFbPitch + 12 * kFbTile, "LDS bytes");
    std::vector<uint8_t> staged((size_t)rows, 0);
    for (int64_t blk = 0; blk < nblk; ++blk) {
        if (blk >= 3 && blk + 3 < nblk) { blk = nblk - 4; continue; }                 // (the first and the last three workgroups)
        const int64_t r0 = blk * kFbRun, rend = r0 + kFbRun < rows ? r0 + kFbRun : rows;
        for (int64_t tr0 = r0; tr0 < rend; tr0 += kFbTile) {
            const int nrow = (int)(rend - tr0 < kFbTile ? rend - tr0 : kFbTile);
            EXPECT(nrow >= 1 && nrow <= kFbTile, "tile rows");
            std::vector<int> wrote((size_t)fb_lds_values(), 0);
            for (int t = 0; t < kFbThreads; ++t)
                for (int k = 0; k < fb_stage_passes(); ++k) {
                    const int r = fb_stage_row(t, k), g = fb_stage_group(t);
                    EXPECT(r >= 0 && r < kFbTile && g >= 0 && g < kFbPitch, "staging map t=%d k=%d", t, k);
                    EXPECT(fb_stage_row(t, k) == fb_stage_row(t & ~63, k), "a wave stages one row t=%d", t);
                    if (r >= nrow) continue;
                    const int li = fb_lds_index(r, g);
                    EXPECT(li >= 0 && li < fb_lds_values(), "LDS write t=%d k=%d", t, k);
                    if (li >= 0 && li < fb_lds_values()) wrote[(size_t)li]++;
                    if (g < P) {
                        const int64_t ci = gc_counts_index(tr0 + r, P, g, 0);
                        EXPECT(ci >= 0 && ci + 3 <= ccap, "counts read rows=%lld P=%d row=%lld g=%d", (long long)rows, P, (long long)(tr0 + r), g);
                    }
                    if ((t & 63) == 0) {
                        EXPECT(tr0 + r >= 0 && tr0 + r < bcap, "block id read row=%lld", (long long)(tr0 + r));
                        if (tr0 + r < rows) staged[(size_t)(tr0 + r)]++;
                    }
                }
            // every (row, group) word a pair can read was written exactly once in this tile
            bool once = true;
            for (int r = 0; r < nrow; ++r)
                for (int g = 0; g < kFbPitch; ++g) once = once && wrote[(size_t)fb_lds_index(r, g)] == 1;
            EXPECT(once, "every LDS word of the tile's rows is staged once rows=%lld", (long long)rows);
            for (int r = 0; r < nrow; r += (nrow > 2 ? nrow - 1 : 1))
                for (int q = 0; q < fb_pairs(P); ++q) {
                    const int ii = fb_lds_index(r, fb_pair_i(q)), jj = fb_lds_index(r, fb_pair_j(q));
                    EXPECT(ii >= 0 && ii < fb_lds_values() && jj >= 0 && jj < fb_lds_values() && ii / kFbPitch == r && jj / kFbPitch == r, "LDS read q=%d", q);
                }
        }
    }
    if (nblk <= 6) {
        bool once = true;
        for (uint8_t v : staged) once = once && v == 1;
        EXPECT(once, "every row is staged by exactly one wave rows=%lld", (long long)rows);
    }
    // the flush: block b in 0 .. B - 1 (the host refuses others), pair q < pairs
    for (int64_t b : {(int64_t)0, B / 2, B - 1})
        for (int q : {0, fb_pairs(P) / 2, fb_pairs(P) - 1}) {
            const int64_t ix = fb_out_index(b, P, q);
            EXPECT(ix >= 0 && ix < ocap, "output index B=%lld P=%d", (long long)B, P);
        }
    EXPECT(fb_out_index(B - 1, P, fb_pairs(P) - 1) == ocap - 1, "the last output is the buffer's last B=%lld P=%d", (long long)B, P);
}

int main() {
    static_assert(kFbThreads == 256 && kFbTile == 32 && kFbRun == 256 && kFbPitch == 64 && kFbSlots == 8, "the shapes the tests name");
    for (int P = 2; P <= kGcMaxGroups; ++P) audit_pairs(P);
    EXPECT(fb_pairs(kGcMaxGroups) == 2016 && fb_slots(kGcMaxGroups) == 8 && fb_slots(23) == 1 && fb_slots(24) == 2, "pairs at the edges");
    const std::vector<int64_t> Rs = {1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 600, 1000, 5000, kFbMaxRows - 1, kFbMaxRows};
    for (int P : {2, 3, 5, 23, 24, 31, 32, 33, 63, 64})
        for (int64_t rows : Rs)
            for (int64_t B : {(int64_t)1, (int64_t)7, rows}) audit_rows(rows, P, B);
    // the OOM sum is the allocations: gpca_group_counts' buffers, the block ids (i32), the sums (i64) and the counts (i32)
    for (int64_t N : {(int64_t)1, (int64_t)257, (int64_t)10000, ((int64_t)1 << 30) - 1})
        for (int P : {2, 33, 64})
            for (int64_t rows : {(int64_t)1, (int64_t)257, kFbMaxRows})
                for (int64_t B : {(int64_t)1, (int64_t)600, kFbMaxRows}) {
                    const double sum = gc_call_bytes(N, rows, P) + 4.0 * (double)fb_block_capacity(rows) + 8.0 * (double)fb_out_capacity(B, P) +
                                       4.0 * (double)fb_out_capacity(B, P);
                    EXPECT(sum == fb_call_bytes(N, rows, P, B), "OOM sum N=%lld rows=%lld P=%d B=%lld", (long long)N, (long long)rows, P, (long long)B);
                    EXPECT(fb_out_capacity(B, P) > 0 && fb_out_capacity(B, P) < ((int64_t)1 << 62) / 8, "output elements fit in 64 bits");
                }
    // the 2^63 bound: |v| <= 1.5 (d d <= 1; each correction is at most 1/4 / 1), so |q| <= 1.5 x 2^40 and a call of kFbMaxRows rows sums
    // to at most 1.5 x 2^61 < 2^63; a count is at most kFbMaxRows < 2^31
    const long double qmax = 1.5L * (long double)kFbScale;
    EXPECT(kFbScale == std::ldexp(1.0, 40), "the grid is 2^-40");
    EXPECT(qmax * (long double)kFbMaxRows < std::ldexp(1.0L, 63), "a call's sums stay below 2^63");
    EXPECT(qmax * (long double)(2 * kFbMaxRows) < std::ldexp(1.0L, 63), "... with a factor of 2 to spare");
    EXPECT(kFbMaxRows < ((int64_t)1 << 31) - 1, "a call's counts fit in i32");
    // the extreme v: p_i = 1, p_j = 0 gives d d = 1 with both corrections 0; p = 1/2 in both with n = 2 gives -(1/4) - (1/4)
    {
        const double v1 = (1.0 * 1.0 - (1.0 * (1.0 - 1.0)) / (2.0 - 1.0)) - (0.0 * (1.0 - 0.0)) / (2.0 - 1.0);
        const double v2 = (0.0 * 0.0 - (0.5 * (1.0 - 0.5)) / (2.0 - 1.0)) - (0.5 * (1.0 - 0.5)) / (2.0 - 1.0);
        EXPECT(v1 == 1.0 && v2 == -0.5 && std::fabs(v1) <= 1.5 && std::fabs(v2) <= 1.5, "the extreme values of v");
    }
    printf("f2_blocks_plan_audit: %lld checks, %lld failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
