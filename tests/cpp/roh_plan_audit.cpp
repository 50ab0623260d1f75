// Extent audit of the runs-of-homozygosity host arithmetic (genomic_pca_amd/csrc/plan_math.h, the roh_* functions): for every plan
// roh_plan can return over a grid of (rows, N, W, CUs, forced splits) and several layouts of window domains it walks every workgroup of
// the launches (roh.hip) and restates their index arithmetic on the host: every row of the band is decided by exactly one split, with
// the coverage a20 gives it; every halo row and every second fetch stays inside the band and inside its domain; every fetch stays
// inside the row's pitch of both storages (gpca_residency.cpp) with the alignment its vector load needs; every plane and count entry
// is written exactly once and read inside its capacity; the GPCA_ERR_OOM sum equals the allocations; and no counter can wrap.
// Includes the header the engine itself uses.
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

// the samples' side of a launch: fetches, plane and count entries of every thread (independent of the rows)
static void audit_samples(int64_t rows, int64_t N, const RohPlan& p) {
    const int64_t npad = roh_npad(N), pitch = roh_plane_pitch(N);
    const int64_t ld8 = (N + kSamplePad - 1) / kSamplePad * kSamplePad, ld2 = (N + 1023) / 1024 * 1024 / 4;
    EXPECT(npad >= N && npad - N < kScLane && npad % kScLane == 0 && npad <= ld8 && npad <= 4 * ld2, "npad N=%lld", (long long)N);
    EXPECT(pitch * 8 == npad && pitch % 2 == 0, "pitch N=%lld", (long long)N);
    EXPECT(p.chunks == sc_chunks(N) && p.chunks * kScChunk >= npad && (p.chunks - 1) * kScChunk < npad, "chunks N=%lld", (long long)N);
    EXPECT(p.splits >= 1 && p.per >= 1 && p.splits <= rows && p.splits * p.per >= rows && (p.splits - 1) * p.per < rows,
           "splits rows=%lld splits=%lld per=%lld", (long long)rows, (long long)p.splits, (long long)p.per);
    const int64_t pcap = roh_plane_capacity(rows, N), ccap = roh_cnt_capacity(p.splits, N), rcap = roh_rec_capacity(p.splits, N);
    std::vector<uint8_t> owner((size_t)npad, 0), prow((size_t)pitch, 0), cw((size_t)ccap, 0);
    bool inside = true;
    for (int64_t chunk = 0; chunk < p.chunks; ++chunk)
        for (int t = 0; t < kScThreads; ++t) {
            const int64_t n0 = sc_thread_sample(chunk, t);
            if (n0 >= npad) continue;
            const int64_t o8 = sc_row_offset(false, n0), o2 = sc_row_offset(true, n0);
            EXPECT(o8 >= 0 && o8 + 16 <= ld8 && o8 % 16 == 0, "int8 fetch N=%lld n0=%lld", (long long)N, (long long)n0);
            EXPECT(o2 >= 0 && o2 + 4 <= ld2 && o2 % 4 == 0, "2-bit fetch N=%lld n0=%lld", (long long)N, (long long)n0);
            EXPECT(N - n0 >= 1, "a live thread owns a sample N=%lld n0=%lld", (long long)N, (long long)n0);
            for (int s = 0; s < kScLane; ++s) owner[(size_t)(n0 + s)]++;
            // the two plane bytes of a row, first and last row of the band
            const int64_t b0 = roh_plane_index(0, pitch, n0), b1 = roh_plane_index(rows - 1, pitch, n0);
            EXPECT(b0 % 2 == 0 && b0 >= 0 && b0 + 2 <= pitch && b1 % 2 == 0 && b1 + 2 <= pcap, "plane bytes N=%lld n0=%lld", (long long)N, (long long)n0);
            prow[(size_t)b0]++; prow[(size_t)b0 + 1]++;
            // the count entries: 16 u32 as four aligned uint4, every split
            for (int64_t split = 0; split < p.splits; split += (p.splits > 64 ? p.splits / 16 : 1)) {
                const int64_t c0 = roh_cnt_index(split, npad, n0);
                EXPECT(c0 % 4 == 0, "count alignment n0=%lld", (long long)n0);
                // the thread's 16 entries of rec: 8 u32 each, as two aligned uint4, inside the buffer; k_roh_stitch reads the same
                const int64_t r0 = roh_rec_index(split, npad, n0), r1 = roh_rec_index(split, npad, n0 + kScLane - 1) + kRohRecWords;
                EXPECT(r0 % 4 == 0 && kRohRecWords == 8 && r0 >= 0 && r1 <= rcap && r1 - r0 == kScLane * kRohRecWords, "rec entries n0=%lld", (long long)n0);
                for (int s = 0; s < kScLane; ++s) {
                    const int64_t ix = c0 + s;
                    if (ix < 0 || ix >= ccap) { inside = false; continue; }
                    if (cw[(size_t)ix] < 255) cw[(size_t)ix]++;
                }
            }
        }
    EXPECT(inside, "a count write leaves its buffer rows=%lld N=%lld splits=%lld", (long long)rows, (long long)N, (long long)p.splits);
    bool once = true;
    for (uint8_t v : owner) once = once && v == 1;
    for (uint8_t v : prow) once = once && v == 1;
    if (p.splits <= 64) for (uint8_t v : cw) once = once && v == 1;
    EXPECT(once, "every sample, plane byte and count entry has one writer rows=%lld N=%lld splits=%lld", (long long)rows, (long long)N, (long long)p.splits);
    // k_roh_stitch: thread n < N reads rec (s, n) and reads and writes cnt (s, n) of every split and writes seg_count [n]; the fill pass
    // reads base [n]
    EXPECT(roh_cnt_index(p.splits - 1, npad, N - 1) < ccap && N - 1 < roh_segcount_capacity(N) && N - 1 < roh_base_capacity(N) &&
           roh_brk_capacity(rows) >= rows, "scan pass N=%lld", (long long)N);
    EXPECT(roh_rec_index(p.splits - 1, npad, npad - 1) + kRohRecWords == rcap && (kRohFlagThrough & kRohFlagTail) == 0u, "last rec entry");
    EXPECT(roh_cnt_index(p.splits - 1, npad, npad - 1) == ccap - 1 && roh_plane_index(rows - 1, pitch, npad - 16) + 2 == pcap, "last entries");
}

// the rows' side of the mark launch: the walk of every split over the domains dom [nd + 1], as k_roh_mark makes it
static void audit_rows(int64_t rows, const RohPlan& p, const std::vector<int>& dom, int W) {
    const int nd = (int)dom.size() - 1;
    EXPECT(nd >= 1 && dom[0] == 0 && dom[nd] == rows && roh_dom_capacity(nd) == nd + 1, "domains rows=%lld", (long long)rows);
    std::vector<int> decided((size_t)rows, 0), cov_seen((size_t)rows, -1);
    for (int64_t split = 0; split < p.splits; ++split) {
        const int64_t ka = split * p.per, kb = ka + p.per < rows ? ka + p.per : rows;
        EXPECT(ka < kb && kb <= rows, "empty split %lld rows=%lld", (long long)split, (long long)rows);
        int lo = 0, hi = nd;
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if ((int64_t)dom[mid] <= ka) lo = mid; else hi = mid; }
        int di = lo;
        EXPECT(dom[di] <= ka && ka < dom[di + 1], "the split's first domain rows=%lld ka=%lld", (long long)rows, (long long)ka);
        for (int64_t pa = ka; pa < kb; ++di) {
            EXPECT(di < nd, "domain index rows=%lld", (long long)rows);
            if (di >= nd) return;
            const int64_t d0 = dom[di], d1 = dom[di + 1], pb = kb < d1 ? kb : d1;
            EXPECT(d0 <= pa && pa < pb && pb <= d1, "piece rows=%lld pa=%lld", (long long)rows, (long long)pa);
            if (d1 - d0 < W) {
                for (int64_t j = pa; j < pb; ++j) { decided[(size_t)j]++; cov_seen[(size_t)j] = 0; }
                pa = pb;
                continue;
            }
            const int64_t s_lo = roh_win_lo(d0, pa, W), s_hi = roh_win_hi(d1, pb, W), t_hi = s_hi + W - 1, s_end = d1 - W;
            EXPECT(s_lo >= d0 && s_lo <= pa && s_lo <= s_hi && s_hi <= s_end && pa - s_lo <= W - 1 && t_hi < d1 && t_hi - (pb - 1) <= W - 1,
                   "halo rows=%lld pa=%lld pb=%lld W=%d", (long long)rows, (long long)pa, (long long)pb, W);
            int inwin = 0, counted = 0;                                              // rows the running counts hold; windows the hit counters hold
            int64_t ring[kRohMaxWindow];                                             // the window each ring slot holds
            for (int i = 0; i < kRohMaxWindow; ++i) ring[i] = -1;
            for (int64_t tt = s_lo; tt <= t_hi; ++tt) {
                EXPECT(tt >= 0 && tt < rows && tt >= d0 && tt < d1, "fetch row rows=%lld tt=%lld", (long long)rows, (long long)tt);
                ++inwin;
                if (tt - s_lo >= W) { EXPECT(tt - W >= d0 && tt - W >= s_lo, "second fetch rows=%lld tt=%lld", (long long)rows, (long long)tt); --inwin; }
                EXPECT(inwin <= W && inwin + 1 <= 255, "byte counter W=%d", W);
                if (tt - s_lo < W - 1) continue;
                EXPECT(inwin == W, "a complete window holds W rows W=%d", W);
                const int64_t s = tt - W + 1;
                if (s - W >= s_lo) {                                                 // read before the slot is reused (W = 64: the same slot)
                    EXPECT(ring[(s - W) & (kRohMaxWindow - 1)] == s - W, "the ring still holds the leaving window rows=%lld s=%lld W=%d", (long long)rows, (long long)s, W);
                    --counted;
                }
                ring[s & (kRohMaxWindow - 1)] = s;
                ++counted;
                if (s >= pa) {
                    EXPECT(s < pb, "decided row inside the piece rows=%lld j=%lld", (long long)rows, (long long)s);
                    const int64_t clo = roh_cov_lo(d0, s, W), cov = s - clo + 1;
                    // the hit counters hold windows max(s_lo, s - W + 1) .. s: exactly the covering windows
                    EXPECT(roh_cov_hi(d1, s, W) == s && clo >= s_lo && cov >= 1 && cov <= W && counted == cov, "coverage rows=%lld j=%lld W=%d", (long long)rows, (long long)s, W);
                    if (s < pb) { decided[(size_t)s]++; cov_seen[(size_t)s] = (int)cov; }
                }
            }
            if (s_hi == s_end)
                for (int64_t j = s_end + 1; j < pb; ++j) {
                    if (j - W >= s_lo) {
                        EXPECT(ring[(j - W) & (kRohMaxWindow - 1)] == j - W, "the ring still holds the leaving window (tail) rows=%lld j=%lld W=%d", (long long)rows, (long long)j, W);
                        --counted;
                    }
                    if (j >= pa) {
                        const int64_t clo = roh_cov_lo(d0, j, W), cov = s_end - clo + 1;
                        EXPECT(roh_cov_hi(d1, j, W) == s_end && clo >= s_lo && cov >= 1 && cov <= W && counted == cov, "tail coverage rows=%lld j=%lld W=%d", (long long)rows, (long long)j, W);
                        decided[(size_t)j]++;
                        cov_seen[(size_t)j] = (int)cov;
                    }
                }
            pa = pb;
        }
    }
    bool once = true, covok = true;
    for (int64_t j = 0; j < rows; ++j) once = once && decided[(size_t)j] == 1;
    // a20 step 2, restated: row j of a domain of L rows is covered by windows max(0, j - W + 1) .. min(j, L - W)
    for (int d = 0; d < nd; ++d) {
        const int64_t L = dom[d + 1] - dom[d];
        for (int64_t j = 0; j < L; ++j) {
            const int64_t a = j - W + 1 > 0 ? j - W + 1 : 0, b = j < L - W ? j : L - W;
            covok = covok && cov_seen[(size_t)(dom[d] + j)] == (int)(b >= a ? b - a + 1 : 0);
        }
    }
    EXPECT(once, "every row decided exactly once rows=%lld splits=%lld W=%d", (long long)rows, (long long)p.splits, W);
    EXPECT(covok, "every row's coverage is a20's rows=%lld splits=%lld W=%d", (long long)rows, (long long)p.splits, W);
    // k_roh_runs: split [ka, kb) reads plane rows ka - 1 (ka > 0) .. kb (kb < rows) and brk rows ka .. kb (kb < rows; never row 0)
    for (int64_t split = 0; split < p.splits; ++split) {
        const int64_t ka = split * p.per, kb = ka + p.per < rows ? ka + p.per : rows;
        EXPECT((ka == 0 || ka - 1 >= 0) && kb <= rows && (kb == rows) == (split == p.splits - 1), "runs walk rows=%lld split=%lld", (long long)rows, (long long)split);
    }
}

static std::vector<int> make_domains(int64_t rows, int W, int layout, std::mt19937_64& rng) {
    std::vector<int> dom{0};
    if (layout == 1) { for (int64_t j = 1; j < rows; ++j) dom.push_back((int)j); }                        // every row a domain
    else if (layout == 2) {                                                                               // lengths around W
        const int lens[5] = {W - 1, W, W + 1, 2 * W - 1, 2 * W};
        int64_t at = 0;
        for (int i = 0;; ++i) { const int L = lens[i % 5] > 0 ? lens[i % 5] : 1; at += L; if (at >= rows) break; dom.push_back((int)at); }
    } else if (layout == 3) { for (int64_t j = 1; j < rows; ++j) if (rng() % 37 == 0) dom.push_back((int)j); }
    dom.push_back((int)rows);
    return dom;
}

int main() {
    // a window's byte count is at most W + 1 <= 65 while a row enters (compared after the leaving row is taken off, at most W <= 64 <
    // 0x80: the compare borrows nothing); hits den and num cov are at most 64 x 2^20 < 2^32; the runs' byte counters are flushed
    // every kRohFlushRows <= 255 fetched rows; a run's u32 counts are at most rows < 2^31; a record index is a u64
    static_assert(kRohMaxWindow == 64 && kRohMaxWindow + 1 < 0x80 && (int64_t)kRohMaxWindow * kRohMaxDen < ((int64_t)1 << 32) && kRohFlushRows <= 255 &&
                  kScLane == 16, "counters");
    std::mt19937_64 rng(20);
    std::vector<int64_t> Ns = {1, 2, 15, 16, 17, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 10000};
    std::vector<int64_t> Rs = {1, 2, 5, 49, 50, 51, 63, 64, 65, 99, 100, 127, 128, 129, 255, 256, 257, 511, 600, 1000};
    for (int t = 0; t < 4; ++t) { Ns.push_back(1 + (int64_t)(rng() % 5000)); Rs.push_back(1 + (int64_t)(rng() % 1500)); }
    for (int64_t rows : Rs) {
        std::vector<RohPlan> plans;
        for (int cus : {1, 8, 256, 304}) plans.push_back(roh_plan(rows, 257, cus));
        for (int64_t forced : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)7, rows, rows + 5, (int64_t)1 << 40}) plans.push_back(roh_plan(rows, 257, 256, forced));
        for (const RohPlan& p : plans)
            for (int W : {1, 2, 5, 50, 63, 64})
                for (int layout = 0; layout < 4; ++layout) audit_rows(rows, p, make_domains(rows, W, layout, rng), W);
        for (int64_t N : Ns) {
            for (int cus : {1, 256}) audit_samples(rows, N, roh_plan(rows, N, cus));
            for (int64_t forced : {(int64_t)1, (int64_t)3, rows, rows + 5}) audit_samples(rows, N, roh_plan(rows, N, 256, forced));
        }
    }
    // the OOM sum is the allocations; large shapes: the plan and the extents alone, up to the call's limits
    for (int64_t N : {(int64_t)1, (int64_t)257, (int64_t)100000, (int64_t)1000003})
        for (int64_t rows : {(int64_t)1, (int64_t)1000000, ((int64_t)1 << 31) - 1}) {
            const RohPlan p = roh_plan(rows, N, 256);
            EXPECT(p.splits * p.per >= rows && (p.splits - 1) * p.per < rows && p.splits >= 1 && sc_grid(p) < ((int64_t)1 << 31), "large plan");
            for (int64_t domains : {(int64_t)1, (int64_t)23, rows})
                for (int64_t rec : {(int64_t)0, (int64_t)12345}) {
                    const double sum = (double)roh_plane_capacity(rows, N) + (double)roh_brk_capacity(rows) + 4.0 * (double)roh_dom_capacity(domains) +
                                       4.0 * (double)roh_cnt_capacity(p.splits, N) + 4.0 * (double)roh_rec_capacity(p.splits, N) +
                                       4.0 * (double)roh_segcount_capacity(N) +
                                       8.0 * (double)roh_base_capacity(N) + 4.0 * (double)roh_seg_capacity(rec) + 8.0;
                    EXPECT(sum == roh_call_bytes(N, rows, p.splits, domains, rec), "OOM sum N=%lld rows=%lld", (long long)N, (long long)rows);
                }
            EXPECT(roh_plane_capacity(rows, N) > 0 && roh_plane_index(rows - 1, roh_plane_pitch(N), roh_npad(N) - 16) + 2 == roh_plane_capacity(rows, N), "plane fits 63 bits");
            EXPECT(roh_dom_capacity(rows) - 1 <= ((int64_t)1 << 31) - 1, "a domain's first row fits an int");
        }
    printf("roh_plan_audit: %lld checks, %lld failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
