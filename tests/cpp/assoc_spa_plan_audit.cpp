// Extent audit of the saddle-point correction's host arithmetic (genomic_pca_amd/csrc/plan_math.h, the asp_* functions): a brute-force
// walk of k_assoc_spa's index arithmetic (assoc_spa.hip) over sample counts at the stage, chunk and slice edges and at their limits:
// every 32-sample word below asp_gpad(N) is fetched once, inside the row's pitch and with its include word; every sample below
// asp_gpad(N) is owned by one thread of one chunk, whose byte lies in the LDS buffer and was written by that chunk's fetches; the
// slices of g~, Z, mu hold every index their readers and writers reach and the slices together stay inside the bound; the ranges of
// the item list cover a band's items once and a range's items fit the list.  Includes the header the engine itself uses.
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

// the sample axis of one item, walked thread by thread (walk = false: the first and the last chunk only, for sample counts too large
// to walk)
static void audit_samples(int64_t N, bool walk) {
    const int64_t npad = asp_gpad(N), chunks = asp_chunks(N);
    EXPECT(npad >= N && npad % 32 == 0 && npad == asc_npad(N), "gpad N=%lld", (long long)N);
    EXPECT(chunks * kAspChunk >= npad && (chunks - 1) * kAspChunk < npad, "chunks N=%lld", (long long)N);
    const int64_t ld8 = (N + kSamplePad - 1) / kSamplePad * kSamplePad, ld2 = (N + 1023) / 1024 * 1024 / 4;
    std::vector<int> fetched(walk ? (size_t)(npad / 32) : 0, 0), owned(walk ? (size_t)npad : 0, 0);
    for (int64_t c = 0; c < chunks; ++c) {
        if (!walk && c != 0 && c != chunks - 1) continue;
        const int64_t c0 = c * kAspChunk;
        std::vector<int> written((size_t)kAspChunk, 0);
        for (int tid = 0; tid < kAspThreads; ++tid) {
            const int64_t n0 = c0 + 32 * tid;
            if (n0 >= npad) continue;
            EXPECT(n0 % 32 == 0 && (n0 >> 5) < asc_inc_capacity(N), "include word N=%lld n0=%lld", (long long)N, (long long)n0);
            EXPECT(n0 + 32 <= ld8 && (n0 >> 2) + 8 <= ld2 && n0 % 16 == 0 && (n0 >> 2) % 8 == 0, "fetch past the pitch N=%lld n0=%lld", (long long)N, (long long)n0);
            EXPECT(32 * tid + 31 < kAspChunk, "LDS write tid=%d", tid);
            for (int b = 0; b < 32; ++b) written[(size_t)(32 * tid + b)] = 1;
            if (walk) fetched[(size_t)(n0 >> 5)]++;
        }
        for (int tid = 0; tid < kAspThreads; ++tid)
            for (int k = 0; k < 32; ++k) {
                const int64_t n = c0 + tid + (int64_t)kAspThreads * k;
                if (n >= npad) break;
                const int l = tid + kAspThreads * k;
                EXPECT(l < kAspChunk && written[(size_t)l] == 1 && c0 + l == n, "LDS read N=%lld n=%lld", (long long)N, (long long)n);
                if (walk) owned[(size_t)n]++;
            }
    }
    if (walk) {
        for (int64_t w = 0; w < npad / 32; ++w) EXPECT(fetched[(size_t)w] == 1, "word %lld fetched %d times N=%lld", (long long)w, fetched[(size_t)w], (long long)N);
        for (int64_t n = 0; n < npad; ++n) EXPECT(owned[(size_t)n] == 1, "sample %lld owned %d times N=%lld", (long long)n, owned[(size_t)n], (long long)N);
    }
    // the passes of the root rule: thread tid reads tid + kAspThreads k below npad: inside the slice
    const int64_t slots = asp_slots(N);
    EXPECT(slots >= 1 && slots <= kAspMaxSlots, "slots N=%lld", (long long)N);
    EXPECT((slots - 1) * npad + (npad - 1) < asp_g_capacity(N), "g~ slices N=%lld", (long long)N);
    EXPECT(8 * asp_g_capacity(N) <= kAspWsBytes || slots == 1, "workspace bound N=%lld", (long long)N);
    EXPECT(slots == kAspMaxSlots || 8 * (slots + 1) * npad > kAspWsBytes, "slots not maximal N=%lld", (long long)N);
    // a forced workgroup count (GPCA_ASP_SLOTS through asp_clamp_slots): in range, the identity on legal values, the default for unset
    // or <= 0, and the slice of its last workgroup inside the workspace, which keeps the size asp_slots(N) gives it
    for (int64_t want : {(int64_t)-7, (int64_t)0, (int64_t)1, (int64_t)2, (int64_t)3, slots - 1, slots, slots + 1, (int64_t)kAspMaxSlots,
                         (int64_t)kAspMaxSlots + 1, (int64_t)1 << 40}) {
        const int64_t got = asp_clamp_slots(N, want);
        EXPECT(got >= 1 && got <= slots, "clamped slots N=%lld want=%lld", (long long)N, (long long)want);
        EXPECT(got == (want >= 1 && want <= slots ? want : slots), "clamp N=%lld want=%lld got=%lld", (long long)N, (long long)want, (long long)got);
        EXPECT((got - 1) * npad + (npad - 1) < asp_g_capacity(N), "forced slices N=%lld want=%lld", (long long)N, (long long)want);
    }
    for (int Pc : {0, 1, 3, 29, 61}) {
        const int T = asr_max_traits(Pc), P = Pc + 1;
        EXPECT(((int64_t)(T - 1) * P + (P - 1)) * npad + (npad - 1) < asp_z_capacity(N, T, Pc), "Z N=%lld Pc=%d", (long long)N, Pc);
        EXPECT((int64_t)(T - 1) * npad + (npad - 1) < asp_mu_capacity(N, T), "mu N=%lld Pc=%d", (long long)N, Pc);
        EXPECT(P <= kAsrMaxCols, "a_j in LDS Pc=%d", Pc);
    }
}

// the items of a band: the ranges cover them once, a range fits the list, the last item's result fits out
static void audit_items(int64_t rows, int T) {
    const int64_t items = rows * (int64_t)T, nr = asp_ranges(rows, T);
    int64_t covered = 0, expect0 = 0;
    for (int64_t item0 = 0; item0 < items; item0 += kAspListItems) {
        const int64_t n = items - item0 < kAspListItems ? items - item0 : kAspListItems;
        EXPECT(item0 == expect0 && n >= 1 && n <= asp_list_capacity(rows, T) && n - 1 < ((int64_t)1 << 31), "range rows=%lld T=%d", (long long)rows, T);
        EXPECT((n + 255) / 256 < ((int64_t)1 << 31), "flag grid rows=%lld T=%d", (long long)rows, T);
        covered += n; expect0 = item0 + n;
        const int64_t last = item0 + n - 1, i = last / T, t = last - i * T;
        EXPECT(i < rows && t < T && last * 4 + 3 < asp_out_capacity(rows, T) && last * 5 + 2 < asr_stats_capacity(rows, T), "last item rows=%lld T=%d", (long long)rows, T);
    }
    EXPECT(covered == items && (items + kAspListItems - 1) / kAspListItems == nr, "ranges rows=%lld T=%d", (long long)rows, T);
}

int main() {
    static_assert(kAspChunk == 32 * kAspThreads && kAspThreads % 64 == 0 && kAspThreads / 64 == 4, "a thread fetches 32 samples; four waves");
    std::mt19937_64 rng(14);
    std::vector<int64_t> Ns = {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 8191, 8192, 8193,
                               10000, 16383, 16384, 16385, 32767, 32768, 32769, 50000, 65537};
    for (int t = 0; t < 40; ++t) Ns.push_back(1 + (int64_t)(rng() % 70000));
    for (int64_t N : Ns) audit_samples(N, true);
    std::vector<int64_t> big = {500000, ((int64_t)1 << 25) - 1, (int64_t)1 << 25, ((int64_t)1 << 25) + 1, ((int64_t)1 << 30) - 1};
    for (int t = 0; t < 200; ++t) big.push_back(1 + (int64_t)(rng() % ((uint64_t)1 << 30)));
    for (int64_t N : big) audit_samples(N, false);
    // the slot classes the lists above hold: all of kAspMaxSlots, fewer (from asp_gpad(N) > 32768 on), one
    EXPECT(asp_slots(32768) == kAspMaxSlots && asp_slots(32769) == 1022 && asp_slots(65537) < kAspMaxSlots && asp_slots(500000) > 1, "slot classes");
    EXPECT(asp_slots(((int64_t)1 << 24) + 1) == 1 && asp_slots((int64_t)1 << 25) == 1 && asp_slots(((int64_t)1 << 30) - 1) == 1, "one slot");
    EXPECT(asp_clamp_slots(32769, 1023) == 1022 && asp_clamp_slots(32769, 3) == 3 && asp_clamp_slots((int64_t)1 << 25, 3) == 1, "clamp at the classes");
    audit_samples(((int64_t)1 << 24) + 1, false);
    std::vector<int64_t> Ks = {1, 2, 127, 128, 129, 4097, kAspListItems - 1, kAspListItems, kAspListItems + 1, 3 * kAspListItems, 1000003, ((int64_t)1 << 31) - 1};
    for (int t = 0; t < 200; ++t) Ks.push_back(1 + (int64_t)(rng() % 30000000));
    for (int64_t K : Ks)
        for (int T : {1, 2, 3, 7, 21}) audit_items(K, T);
    printf("assoc_spa_plan_audit: %lld checks, %lld failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
