// Extent audit of the LD-score host arithmetic (genomic_pca_amd/csrc/plan_math.h, the ld_score_* functions): for band sizes up to 10^7
// rows and window widths up to 2^20 slots, at the tile edges and at seeded random values, every writer of k_ld_score (ld.hip) stays
// inside the buffers gpca_ld_score.cpp allocates, the grid covers every slot of the band exactly once, every pair's partner belongs to
// exactly one thread of its tile, and the packed (count, sum) words and the 64-bit sums cannot overflow.  Restates the kernel's index
// arithmetic on the host; includes the header the engine itself uses.
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

// the tile and the thread of k_ld_score that hold slot (t, d), as the kernel finds them: tile (t / rows-per-tile, d / slots-per-tile),
// thread p = lt + dl reading in step lt
struct Owner { int64_t block, p, lt; };
static Owner owner_of(int64_t t, int64_t d, int64_t nrt) {
    const int64_t rt = t / kLdScoreRows, dt = d / kLdScoreSlots, lt = t % kLdScoreRows, dl = d % kLdScoreSlots;
    return {rt + nrt * dt, lt + dl, lt};
}

static void audit_band(int64_t K, int64_t row0, int64_t rows, int64_t wmax, int64_t weff) {
    const int64_t row1 = row0 + rows;
    const int64_t span = ld_score_span(K, row0, row1, wmax);
    const int64_t cap_a = ld_score_acc_capacity(K, row0, row1, wmax), cap_p = ld_score_partners_capacity(K, row0, row1, wmax);
    EXPECT(span >= rows && span <= rows + wmax && row0 + span <= K, "span K=%lld row0=%lld rows=%lld wmax=%lld", (long long)K, (long long)row0, (long long)rows, (long long)wmax);
    EXPECT(cap_a >= span && cap_p >= span, "capacities below the span rows=%lld wmax=%lld", (long long)rows, (long long)wmax);
    const int64_t nrt = ld_score_row_tiles(rows), ndt = ld_score_slot_tiles(weff), grid = ld_score_grid(rows, weff);
    EXPECT(nrt * kLdScoreRows >= rows && (nrt - 1) * kLdScoreRows < rows, "row tiles rows=%lld", (long long)rows);
    EXPECT(ndt * kLdScoreSlots >= weff && (ndt - 1) * kLdScoreSlots < weff, "slot tiles weff=%lld", (long long)weff);
    EXPECT(grid == nrt * ndt && grid < ((int64_t)1 << 31), "grid rows=%lld weff=%lld", (long long)rows, (long long)weff);
    // the stat rows gpca_ld_score.cpp allocates: [row0, hi), hi = the furthest window end
    const int64_t hi = std::max(row1, std::min(K, row1 - 1 + weff + 1)), nstat = hi - row0;
    EXPECT(nstat <= span, "stat rows beyond the span rows=%lld weff=%lld wmax=%lld", (long long)rows, (long long)weff, (long long)wmax);
    // slots at the corners and edges of the band and of its tiles: one owner each, its reads and its two targets inside the buffers
    const int64_t plane = rows * wmax;
    for (int64_t t : {(int64_t)0, (int64_t)kLdScoreRows - 1, (int64_t)kLdScoreRows, rows / 2, rows - 1}) {
        if (t < 0 || t >= rows) continue;
        for (int64_t d : {(int64_t)0, (int64_t)kLdScoreSlots - 1, (int64_t)kLdScoreSlots, weff / 2, weff - 1}) {
            if (d < 0 || d >= weff) continue;
            const int64_t j = row0 + t + 1 + d;
            if (j >= K) continue;                                        // (win_end <= K: never valid)
            const Owner o = owner_of(t, d, nrt);
            EXPECT(o.block < grid, "slot (%lld, %lld) beyond the grid", (long long)t, (long long)d);
            EXPECT(o.p >= 0 && o.p < kLdScoreThreads - 1, "slot (%lld, %lld): thread %lld", (long long)t, (long long)d, (long long)o.p);
            // the kernel's own arithmetic, from the owner back to the slot and to the partner row
            const int64_t t0 = (o.block % nrt) * kLdScoreRows, d0 = (o.block / nrt) * kLdScoreSlots;
            const int64_t jr = t0 + d0 + 1 + o.p, dl = o.p - o.lt;
            EXPECT(t0 + o.lt == t && d0 + dl == d && dl >= 0 && dl < kLdScoreSlots, "slot (%lld, %lld) is not the owner's", (long long)t, (long long)d);
            EXPECT(row0 + jr == j, "partner of slot (%lld, %lld)", (long long)t, (long long)d);
            EXPECT(jr < nstat && 3 * jr + 2 < ld_stat_capacity(row0, hi), "stat read of partner %lld", (long long)jr);
            EXPECT(t * wmax + d < plane && (kLdProducts - 1) * plane + t * wmax + d < ld_ws_capacity(rows, wmax), "plane read (%lld, %lld)", (long long)t, (long long)d);
            EXPECT(jr < cap_a && jr < cap_p && t < cap_a && t < cap_p, "targets of slot (%lld, %lld): %lld of %lld", (long long)t, (long long)d, (long long)jr, (long long)cap_a);
        }
    }
}

int main() {
    static_assert(kLdScoreThreads == kLdScoreRows + kLdScoreSlots && kLdScoreThreads % 64 == 0 && kLdScoreThreads <= 1024, "one thread per anti-diagonal");
    // a packed word holds at most kLdScoreSlots pairs (a row's own sum over the tile; a partner's holds kLdScoreRows): the sum field is
    // signed and kLdScoreCountShift bits wide, the count sits above it
    static_assert((int64_t)kLdScoreSlots * ((int64_t)1 << 40) < ((int64_t)1 << (kLdScoreCountShift - 1)), "sum field of a packed word");
    static_assert(kLdScoreRows <= kLdScoreSlots && (int64_t)kLdScoreSlots < ((int64_t)1 << (63 - kLdScoreCountShift)), "count field of a packed word");
    // a row is in at most 2 wmax pairs, each |q| <= 2^40 + 2^40 (unbiased v >= -1 at n = 3): below 2^63
    static_assert(2.0 * kLdScoreMaxWmax * 2199023255552.0 < 9223372036854775808.0, "64-bit sums at the largest wmax");
    std::mt19937_64 rng(11);
    std::vector<int64_t> Rs = {1, 2, 63, 64, 65, 127, 128, 129, 4096, 1000003, 10000000};
    std::vector<int64_t> Ws = {1, 2, 63, 64, 65, 255, 256, 257, 319, 320, 321, 511, 512, 513, 1000, 4097, 65536, (1 << 20) - 1, 1 << 20};
    for (int t = 0; t < 200; ++t) { Rs.push_back(1 + (int64_t)(rng() % 10000000)); Ws.push_back(1 + (int64_t)(rng() % (1 << 20))); }
    for (int64_t rows : Rs)
        for (int64_t wmax : Ws)
            for (int64_t weff : {(int64_t)1, wmax / 2, wmax - 1, wmax}) {
                if (weff < 1) continue;
                for (int64_t row0 : {(int64_t)0, (int64_t)77}) {
                    audit_band(row0 + rows + wmax + 5, row0, rows, wmax, weff);     // windows never reach K
                    audit_band(row0 + rows + weff / 2, row0, rows, wmax, weff);     // K cuts the last windows
                    audit_band(row0 + rows, row0, rows, wmax, weff);                // the band ends at K
                }
            }
    printf("ld_score_plan_audit: %lld checks, %lld failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
