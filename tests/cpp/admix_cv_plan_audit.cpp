// Extent audit of the hold-out step's host arithmetic (genomic_pca_amd/csrc/plan_math.h, the adm_cv_* functions; include/gpca.h section
// a22), in the style of admix_plan_audit.cpp, which audits everything the plain step shares with it.  Over the same grid of (rows, N, K):
// the [partial][2] slab llpart of k_admix_step<*, *, true> -- every entry written exactly once, by thread 0 of its workgroup, and read
// exactly once by k_admix_sum64 with two components, inside the capacity gpca_admix.cpp allocates; the two sums and the two counts inside
// theirs; the GPCA_ERR_OOM sum of a hold-out call against its allocations; and the fold rule's quads: a tile of kAdmTile rows takes
// kAdmTile / 4 philox calls whose quad index (i0 >> 2) + qd is the global quad i >> 2 of each of its rows, whatever the block, and no
// per-thread count can pass 32 bits.  Restates the kernel's index arithmetic on the host; includes the header the engine itself uses.
#include "plan_math.h"

#include <cstdio>
#include <random>
#include <vector>

using namespace gpca;

static long long g_checks = 0, g_fail = 0, g_plans = 0, g_walked = 0;
#define EXPECT(cond, ...)                                                        \
    do {                                                                         \
        ++g_checks;                                                              \
        if (!(cond)) { if (++g_fail <= 20) { printf("FAIL " __VA_ARGS__); printf("\n"); } } \
    } while (0)

static void audit_launch(int64_t rows, int64_t N, int K, bool walk) {
    ++g_plans;
    const AdmPlan p = adm_plan(rows, N);
    const int64_t lcap = adm_llpart_capacity(p), ccap = adm_cv_llpart_capacity(p);
    EXPECT(ccap == 2 * lcap && ccap == 2 * p.blocks * p.chunks, "capacity rows=%lld N=%lld", (long long)rows, (long long)N);
    EXPECT(adm_cv_llpart_index(0, p.chunks, 0, 0) == 0 && adm_cv_llpart_index(p.blocks - 1, p.chunks, p.chunks - 1, 1) == ccap - 1, "first and last entries");
    EXPECT(adm_cv_sums_capacity() == 2 && adm_cv_count_capacity() == 2, "two sums, two counts");
    // the OOM sum is the allocations: adm_alloc with hold = true
    const int64_t fcap = adm_fpart_capacity(p, rows, K), qcap = adm_qpart_capacity(p, N, K);
    for (int sets : {2, 5}) {
        const bool fit = sets == 5;
        const double sum = 4.0 * sets * (double)(N * K) + 4.0 * sets * (double)(rows * K) + (double)N + 4.0 * (double)fcap + 4.0 * (double)qcap +
                           8.0 * (double)ccap + 8.0 * 2 + 8.0 * 2 + (fit ? 8.0 * (double)adm_npart_capacity(N, rows, K) : 0.0) + 3 * 8.0 + 8.0;
        EXPECT(sum == adm_cv_call_bytes(N, rows, K, sets, fit), "OOM sum rows=%lld N=%lld K=%d", (long long)rows, (long long)N, K);
        EXPECT(adm_cv_call_bytes(N, rows, K, sets, fit) == adm_call_bytes(N, rows, K, sets, fit) + 8.0 * (double)lcap + 32.0, "over the plain call");
    }
    if (!walk) return;
    ++g_walked;
    std::vector<uint8_t> lw((size_t)ccap, 0), quad_of((size_t)rows, 0);
    bool inside = true, quads = true;
    for (int64_t w = 0; w < adm_grid(p); ++w) {
        const int64_t chunk = w % p.chunks, block = w / p.chunks;
        const int64_t ka = block * kAdmRowBlock, kb = ka + kAdmRowBlock < rows ? ka + kAdmRowBlock : rows;
        for (int64_t i0 = ka; i0 < kb; i0 += kAdmTile) {
            quads = quads && i0 % kAdmCvQuad == 0;
            for (int qd = 0; qd < kAdmTile / kAdmCvQuad; ++qd)
                for (int x = 0; x < kAdmCvQuad; ++x) {
                    const int64_t i = i0 + qd * kAdmCvQuad + x;                      // register c[qd * 4 + x] of the tile
                    if (i >= kb) continue;
                    quads = quads && ((i0 >> 2) + qd) == (i >> 2) && x == (int)(i & 3);
                    if (chunk == 0) quad_of[(size_t)i]++;
                }
        }
        EXPECT(kb - ka <= kAdmRowBlock && (int64_t)kAdmThreads * kAdmRowBlock < ((int64_t)1 << 32), "a workgroup's counts fit 32 bits");
        for (int comp = 0; comp < 2; ++comp) {
            const int64_t il = adm_cv_llpart_index(block, p.chunks, chunk, comp);
            if (il < 0 || il >= ccap) inside = false; else lw[(size_t)il]++;
        }
    }
    EXPECT(inside, "a slab write leaves its extent rows=%lld N=%lld", (long long)rows, (long long)N);
    EXPECT(quads, "a tile's philox calls are the global quads of its rows rows=%lld", (long long)rows);
    bool once = true;
    for (uint8_t v : quad_of) once = once && v == 1;
    EXPECT(once, "every kept row gets its fold from exactly one word rows=%lld", (long long)rows);
    once = true;
    for (uint8_t v : lw) once = once && v == 1;
    EXPECT(once, "every slab entry written exactly once rows=%lld N=%lld", (long long)rows, (long long)N);
    // k_admix_sum64(part, n = lcap, ncomp = 2): thread t reads part[i * 2 + c] for i = t, t + 256, ... < n
    for (int c = 0; c < 2; ++c)
        for (int t = 0; t < kAdmSumThreads; ++t)
            for (int64_t i = t; i < lcap; i += kAdmSumThreads) {
                const int64_t ix = i * 2 + c;
                if (ix >= 0 && ix < ccap) lw[(size_t)ix]--; else inside = false;
            }
    once = inside;
    for (uint8_t v : lw) once = once && v == 0;
    EXPECT(once, "every slab entry read exactly once rows=%lld N=%lld", (long long)rows, (long long)N);
}

int main() {
    static_assert(kAdmTile % kAdmCvQuad == 0 && kAdmRowBlock % kAdmTile == 0 && kAdmCvQuad == 4, "whole quads in a tile, whole tiles in a block");
    static_assert(kAdmCvMinFolds == 2 && kAdmCvMaxFolds == 64, "a22's range of folds");
    // the fold of a word: below folds for every word, and the ends of the range
    for (uint32_t v = kAdmCvMinFolds; v <= (uint32_t)kAdmCvMaxFolds; ++v) {
        EXPECT(adm_cv_fold_of(0u, v) == 0u && adm_cv_fold_of(0xffffffffu, v) == v - 1u, "fold ends v=%u", v);
        for (uint32_t c = 1; c < v; ++c) {                                           // the first word of fold c: ceil(c 2^32 / v)
            const uint32_t w = (uint32_t)((((uint64_t)c << 32) + v - 1) / v);
            EXPECT(adm_cv_fold_of(w, v) == c && adm_cv_fold_of(w - 1u, v) == c - 1u, "fold boundary v=%u c=%u", v, c);
        }
    }
    std::mt19937_64 rng(22);
    std::vector<int64_t> Ns, Rs;
    for (int64_t v = 1; v <= 70; ++v) { Ns.push_back(v); Rs.push_back(v); }
    for (int64_t c : {(int64_t)kAdmChunk, (int64_t)2 * kAdmChunk, (int64_t)1024, (int64_t)2048}) for (int64_t d = -1; d <= 1; ++d) Ns.push_back(c + d);
    for (int64_t c : {(int64_t)kAdmRowBlock, (int64_t)2 * kAdmRowBlock}) for (int64_t d = -1; d <= 1; ++d) Rs.push_back(c + d);
    for (int64_t c : {(int64_t)63, (int64_t)64, (int64_t)65, (int64_t)100, (int64_t)1000}) { Ns.push_back(c); Rs.push_back(c); }
    while (Ns.size() < 100) Ns.push_back(71 + (int64_t)(rng() % 3000));
    while (Rs.size() < 100) Rs.push_back(71 + (int64_t)(rng() % 9000));
    for (int64_t N : Ns)
        for (int64_t rows : Rs)
            for (int K = 1; K <= kAdmMaxK; ++K) audit_launch(rows, N, K, K == 1 || K == kAdmMaxK);   // (the slab does not depend on K)
    for (int64_t N : {(int64_t)10000, (int64_t)1000003})
        for (int64_t rows : {(int64_t)1, (int64_t)1000000, ((int64_t)1 << 31) - 1}) audit_launch(rows, N, 16, false);
    printf("admix_cv_plan_audit: %lld checks, %lld plans, %lld walked, %lld failures\n", g_checks, g_plans, g_walked, g_fail);
    return g_fail ? 1 : 0;
}
