// Extent audit of the Firth correction's host arithmetic (genomic_pca_amd/csrc/plan_math.h: afi_out_capacity, the asp_* functions as
// gpca_assoc_logistic_firth uses them, and asr_call_bytes, the sum of the GPCA_ERR_OOM check).  A brute-force walk of k_assoc_firth's
// and k_assoc_firth_flag's index arithmetic (assoc_firth.hip): every item of a band is flagged once, by a thread of one range, and its
// kAfiWidth results and its z lie inside out and stats; a range's items fit the list; a workgroup's slice of g~ and its trait's Z and
// mu hold every sample a staging thread or a pass reaches (the staging walk itself is k_assoc_spa's: tests/cpp/assoc_spa_plan_audit.cpp);
// the five-value reduction's LDS words lie inside its buffer; and asr_call_bytes equals the sum of the buffers the call allocates,
// restated here in the order of gpca_assoc_score.cpp, for every combination of outputs, with and without a finite cutoff.
// Includes the header the engine itself uses.
#include "plan_math.h"

#include <algorithm>
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

// the items of a band, walked thread by thread of the flag kernel (walk = false: the first and last workgroup of every range)
static void audit_items(int64_t rows, int T, bool walk) {
    const int64_t items = rows * (int64_t)T, out = afi_out_capacity(rows, T), stats = asr_stats_capacity(rows, T);
    EXPECT(out == (int64_t)kAfiWidth * items, "out rows=%lld T=%d", (long long)rows, T);
    int64_t covered = 0, next = 0, ranges = 0;
    for (int64_t item0 = 0; item0 < items; item0 += kAspListItems, ++ranges) {
        const int64_t n = std::min<int64_t>(kAspListItems, items - item0), blocks = (n + 255) / 256;
        EXPECT(n >= 1 && n <= asp_list_capacity(rows, T) && blocks < ((int64_t)1 << 31), "range rows=%lld T=%d", (long long)rows, T);
        for (int64_t b = 0; b < blocks; ++b) {
            if (!walk && b != 0 && b != blocks - 1) { const int64_t k0 = b * 256; covered += std::min<int64_t>(256, n - k0); next = item0 + std::min<int64_t>(n, k0 + 256); continue; }
            for (int tid = 0; tid < 256; ++tid) {
                const int64_t k = b * 256 + tid;
                if (k >= n) continue;
                const int64_t item = item0 + k, i = item / T, t = item - i * T;
                EXPECT(item == next, "item order rows=%lld T=%d item=%lld", (long long)rows, T, (long long)item);
                EXPECT(i < rows && t < T, "row of item %lld rows=%lld T=%d", (long long)item, (long long)rows, T);
                EXPECT(item * 5 + 2 < stats, "z of item %lld rows=%lld T=%d", (long long)item, (long long)rows, T);
                EXPECT(item * kAfiWidth >= 0 && item * kAfiWidth + (kAfiWidth - 1) < out, "out of item %lld rows=%lld T=%d", (long long)item, (long long)rows, T);
                EXPECT(k <= 0x7fffffff && k < asp_list_capacity(rows, T), "list entry k=%lld rows=%lld T=%d", (long long)k, (long long)rows, T);   // (every item flagged)
                // what k_assoc_firth reads of the row: sums [3 i + 1], dv [i L + column], the kept-row index row0 + i
                EXPECT(3 * i + 1 < asr_sums_capacity(rows), "sums row=%lld", (long long)i);
                ++covered; next = item + 1;
            }
        }
    }
    EXPECT(covered == items && ranges == asp_ranges(rows, T), "cover rows=%lld T=%d: %lld of %lld", (long long)rows, T, (long long)covered, (long long)items);
}

// the sample axis as the passes and the slices use it
static void audit_samples(int64_t N) {
    const int64_t npad = asp_gpad(N), slots = asp_slots(N);
    EXPECT(npad >= N && npad % 32 == 0, "gpad N=%lld", (long long)N);
    EXPECT(slots >= 1 && slots <= kAspMaxSlots, "slots N=%lld", (long long)N);
    // a pass: thread tid reads g~ and mu at tid + kAspThreads k below npad; the last workgroup's slice ends inside the workspace
    int64_t last = -1;
    for (int tid = 0; tid < kAspThreads; ++tid) {
        if (tid >= npad) continue;
        const int64_t n = tid + (npad - 1 - tid) / kAspThreads * kAspThreads;
        EXPECT(n < npad && n + kAspThreads >= npad, "last sample of thread %d N=%lld", tid, (long long)N);
        last = std::max(last, n);
    }
    EXPECT(last == npad - 1, "the threads reach the last sample N=%lld", (long long)N);
    EXPECT((slots - 1) * npad + last < asp_g_capacity(N), "g~ slices N=%lld", (long long)N);
    EXPECT(8 * asp_g_capacity(N) <= kAspWsBytes || slots == 1, "workspace bound N=%lld", (long long)N);
    for (int Pc : {0, 1, 3, 29, 61}) {
        const int T = asr_max_traits(Pc), P = Pc + 1;
        EXPECT(((int64_t)(T - 1) * P + (P - 1)) * npad + last < asp_z_capacity(N, T, Pc), "Z N=%lld Pc=%d", (long long)N, Pc);
        EXPECT((int64_t)(T - 1) * npad + last < asp_mu_capacity(N, T), "mu N=%lld Pc=%d", (long long)N, Pc);
        EXPECT(P <= kAsrMaxCols && asr_cols(T, Pc) <= kAsrMaxCols, "a_j in LDS Pc=%d", Pc);
    }
}

// asr_call_bytes against the allocations of gpca_assoc_score.cpp, one line per dalloc
static void audit_bytes(int64_t N, int64_t rows, int T, int Pc) {
    const int L = asr_cols(T, Pc);
    for (int mode = 0; mode < 3; ++mode)                 // none, saddle-point, Firth
        for (int finite = 0; finite < 2; ++finite)
            for (int outs = 0; outs < 8; ++outs) {
                const bool stats = outs & 1, ua = outs & 2, info = outs & 4, with_corr = mode != 0, correct = with_corr && finite;
                const bool dstats = stats || with_corr;
                const int64_t out_cap = mode == 2 ? afi_out_capacity(rows, T) : asp_out_capacity(rows, T);
                double sum = 0.0;
                sum += 4.0 * (double)asc_b_capacity(N, L);                        // Bt (f32)
                sum += 4.0 * (double)asc_inc_capacity(N);                         // incw (u32)
                sum += 8.0;                                                       // bad (u64)
                sum += 8.0 * (double)asr_dv_capacity(rows, L);                    // dv
                sum += 4.0 * (double)asr_sums_capacity(rows);                     // sums (u32)
                if (dstats) sum += 8.0 * (double)asr_stats_capacity(rows, T);
                if (ua) sum += 8.0 * (double)asr_ua_capacity(rows, T, Pc);
                if (info) sum += 8.0 * (double)asr_info_capacity(rows);
                if (with_corr) { sum += 8.0 * (double)out_cap; sum += 4.0 * (double)asp_list_capacity(rows, T); sum += 4.0; }
                if (correct) { sum += 8.0 * (double)asp_z_capacity(N, T, Pc); sum += 8.0 * (double)asp_mu_capacity(N, T); sum += 8.0 * (double)asp_g_capacity(N); }
                const double got = asr_call_bytes(N, rows, T, Pc, dstats, ua, info, with_corr ? out_cap : 0, correct);
                EXPECT(got == sum, "bytes N=%lld rows=%lld T=%d Pc=%d mode=%d finite=%d outs=%d: %.0f != %.0f", (long long)N, (long long)rows, T, Pc, mode,
                       finite, outs, got, sum);
                // +inf: nothing of the correction's inputs is counted
                if (with_corr && !finite)
                    EXPECT(got == asr_call_bytes(N, rows, T, Pc, dstats, ua, info, 0, false) + 8.0 * (double)out_cap + 4.0 * (double)asp_list_capacity(rows, T) + 4.0,
                           "no correction input at +inf N=%lld", (long long)N);
            }
}

int main() {
    static_assert(kAfiWidth == 5, "-log10 p, status, beta, se, D");
    static_assert(kAspThreads / 64 == 4 && 5 * (kAspThreads / 64) == 20, "five values of four waves in the reduction's 20 LDS words");
    std::mt19937_64 rng(15);
    std::vector<int64_t> Ks = {1, 2, 127, 128, 129, 255, 256, 257, 4097, 70000};
    for (int t = 0; t < 20; ++t) Ks.push_back(1 + (int64_t)(rng() % 100000));
    for (int64_t K : Ks)
        for (int T : {1, 2, 3, 7, 16, 21}) audit_items(K, T, true);
    std::vector<int64_t> big = {kAspListItems - 1, kAspListItems, kAspListItems + 1, 3 * kAspListItems, 1000003, ((int64_t)1 << 31) - 1};
    for (int t = 0; t < 100; ++t) big.push_back(1 + (int64_t)(rng() % 30000000));
    for (int64_t K : big)
        for (int T : {1, 2, 3, 7, 16, 21}) audit_items(K, T, false);
    audit_items(70000, 16, true);                           // (the GPU test's walk across the list range)
    std::vector<int64_t> Ns = {1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 8191, 8192, 8193, 10000, 32768, 32769, 65537, 500000,
                               ((int64_t)1 << 25) - 1, (int64_t)1 << 25, ((int64_t)1 << 25) + 1, ((int64_t)1 << 30) - 1};
    for (int t = 0; t < 200; ++t) Ns.push_back(1 + (int64_t)(rng() % ((uint64_t)1 << 30)));
    for (int64_t N : Ns) audit_samples(N);
    for (int64_t N : {(int64_t)1, (int64_t)63, (int64_t)2049, (int64_t)8193, (int64_t)10000, (int64_t)500000})
        for (int64_t rows : {(int64_t)1, (int64_t)130, (int64_t)70000, (int64_t)200000, kAspListItems + 1})
            for (int Pc : {0, 1, 3, 61}) {
                audit_bytes(N, rows, 1, Pc);
                audit_bytes(N, rows, asr_max_traits(Pc), Pc);
            }
    printf("assoc_firth_plan_audit: %lld checks, %lld failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
