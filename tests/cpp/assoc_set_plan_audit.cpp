// Extent audit of the set call's host arithmetic (genomic_pca_amd/csrc/plan_math.h: kAsg*, asg_* and AsgStrip, as
// gpca_assoc_logistic_set sizes its launches and buffers with them).  A brute-force walk of k_assoc_set_gram's and k_assoc_set_finish's
// index arithmetic (assoc_set.hip): for every set size m = 1 .. kAsgMaxRows, every strip, every wave's tile and every accumulator element,
// each entry of the packed lower triangle is written once by the Gram kernel and once by the finish kernel, inside phi; every staged row
// is a listed row of the set, and the tiles read only staged (or zero-filled) LDS rows; the first and last workgroup of large calls keep
// their rows, sums, dv and phi entries inside the buffers; every staged read of a row and of the w column stays inside the row's pitch
// for N up to 2^30 - 1; and asg_call_bytes equals the sum of the buffers the call allocates, restated here in the order of
// gpca_assoc_score.cpp.  Includes the header the engine itself uses.
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

// the row of a 32 x 32 accumulator that element e holds in lane half h (kernels.h: acc_row)
static int acc_row_model(int row0, int e, int h) { return row0 + (e & 3) + 8 * (e >> 2) + 4 * h; }

// the strips of a call as gpca_assoc_score.cpp's set_plan builds them
struct Call { std::vector<AsgStrip> strips; int64_t listed = 0, tri_total = 0; };
static Call plan(const std::vector<int>& ms, int T) {
    Call c;
    for (int m : ms) {
        for (int q = 0; q < asg_strips(m); ++q) c.strips.push_back(AsgStrip{c.listed, c.tri_total * (int64_t)T, m, q});
        c.listed += m; c.tri_total += asg_tri(m);
    }
    return c;
}

// one workgroup (strip, trait) of either kernel, thread by thread: marks the phi entries it writes
static void walk_strip(const Call& c, const AsgStrip& sp, int T, int t, std::vector<unsigned char>* gram, std::vector<unsigned char>* fin) {
    const int64_t phi_cap = asg_phi_capacity(c.tri_total, T), sums_cap = asr_sums_capacity(c.listed);
    const int staged = asg_staged_rows(sp.m, sp.s);
    EXPECT(staged >= 1 && staged <= sp.m && staged <= kAsgMaxRows && kAsgStripRows * sp.s < sp.m, "staged rows m=%d s=%d", sp.m, sp.s);
    // staging: thread tid stages half tid & 1 of the set's row tid / 2
    for (int tid = 0; tid < kAsgThreads; ++tid) {
        const int srow = tid >> 1;
        EXPECT(srow < kAsgMaxRows && (srow + 1) * kAscGPitch <= kAsgMaxRows * kAscGPitch, "LDS row of thread %d", tid);
        if (srow >= staged) continue;
        EXPECT(sp.l0 + srow < asg_rows_capacity(c.listed), "listed row m=%d s=%d srow=%d", sp.m, sp.s, srow);
        EXPECT((sp.l0 + srow) * 3 + 1 < sums_cap, "sums of row m=%d srow=%d", sp.m, srow);
    }
    // the tiles: wave wv <= s, lane (c, h), element e
    for (int wv = 0; wv < kAsgThreads / 64; ++wv) {
        if (wv > sp.s) continue;
        for (int lane = 0; lane < 64; ++lane) {
            const int cc = lane & 31, h = lane >> 5, b = kAsgStripRows * wv + cc;
            // LDS rows the lane reads (a zero-filled row where it lies past the staged ones)
            EXPECT(kAsgStripRows * sp.s + cc < kAsgMaxRows && b < kAsgMaxRows, "LDS rows of lane %d m=%d s=%d wv=%d", lane, sp.m, sp.s, wv);
            for (int e = 0; e < 16; ++e) {
                const int a = acc_row_model(kAsgStripRows * sp.s, e, h);
                if (a >= sp.m || b > a) continue;
                EXPECT(a < staged && b < staged, "an entry's rows are staged m=%d s=%d a=%d b=%d", sp.m, sp.s, a, b);
                const int64_t at = asg_phi_index(sp.p0, sp.m, t, a, b);
                EXPECT(at >= 0 && at < phi_cap, "phi entry m=%d a=%d b=%d t=%d", sp.m, a, b, t);
                if (gram && at >= 0 && at < phi_cap) { EXPECT((*gram)[(size_t)at] == 0, "written twice m=%d a=%d b=%d", sp.m, a, b); (*gram)[(size_t)at] = 1; }
            }
        }
    }
    // the finish kernel: thread tid owns row 32 s + tid / 8 and the columns tid % 8 + 8 k
    for (int tid = 0; tid < 256; ++tid) {
        const int a = kAsgStripRows * sp.s + (tid >> 3);
        if (a >= sp.m) continue;
        EXPECT((sp.l0 + a) * 3 + 1 < sums_cap, "finish: sums a=%d", a);
        for (int b = tid & 7; b <= a; b += 8) {
            const int64_t at = asg_phi_index(sp.p0, sp.m, t, a, b);
            EXPECT(at >= 0 && at < phi_cap && sp.l0 + b < c.listed, "finish: phi entry m=%d a=%d b=%d", sp.m, a, b);
            if (fin && at >= 0 && at < phi_cap) { EXPECT((*fin)[(size_t)at] == 0, "finish: written twice m=%d a=%d b=%d", sp.m, a, b); (*fin)[(size_t)at] = 1; }
        }
    }
}

// a whole call, every workgroup: each entry of phi once in either kernel
static void audit_call(const std::vector<int>& ms, int T) {
    const Call c = plan(ms, T);
    int64_t strips = 0;
    for (int m : ms) strips += asg_strips(m);
    EXPECT((int64_t)c.strips.size() == strips && strips < ((int64_t)1 << 31), "strips");
    std::vector<unsigned char> gram((size_t)asg_phi_capacity(c.tri_total, T), 0), fin(gram.size(), 0);
    for (const AsgStrip& sp : c.strips)
        for (int t = 0; t < T; ++t) walk_strip(c, sp, T, t, &gram, &fin);
    const int64_t g = std::count(gram.begin(), gram.end(), 1), f = std::count(fin.begin(), fin.end(), 1);
    EXPECT(g == (int64_t)gram.size() && f == g, "cover: %lld and %lld of %lld", (long long)g, (long long)f, (long long)gram.size());
    // dv: the last column of the last row the finish kernel reads
    for (int Pc : {0, 1, 29, 61}) {
        if (T > asr_max_traits(Pc)) continue;
        const int L = asr_cols(T, Pc);
        EXPECT((c.listed - 1) * L + asr_col_a(T, Pc, T - 1, Pc) < asr_dv_capacity(c.listed, L), "dv T=%d Pc=%d", T, Pc);
    }
}

// the first and the last workgroups of a large call (the walk above, without the marks)
static void audit_large(int64_t n_sets, int m, int T) {
    Call c;
    c.listed = n_sets * m; c.tri_total = n_sets * asg_tri(m);
    const int64_t strips = n_sets * asg_strips(m);
    EXPECT(strips < ((int64_t)1 << 31), "grid n_sets=%lld m=%d", (long long)n_sets, m);
    for (int64_t set : {(int64_t)0, n_sets - 1})
        for (int q = 0; q < asg_strips(m); ++q) {
            const AsgStrip sp{set * m, set * asg_tri(m) * T, m, q};
            for (int t : {0, T - 1}) walk_strip(c, sp, T, t, nullptr, nullptr);
        }
}

// the sample axis: the staged reads of a row (asc_fetch at a multiple of 32 below npad) and of the w column
static void audit_samples(int64_t N) {
    const int64_t npad = asc_npad(N), nst = asc_stages(N);
    EXPECT(npad >= N && npad % kAscStage == 0 && nst * kAscStage == npad, "npad N=%lld", (long long)N);
    // the rows' pitches in bytes, as the handle lays them out: int8 rows padded to kSamplePad samples, 2-bit rows to 1024 samples
    const int64_t ld8 = (N + kSamplePad - 1) / kSamplePad * kSamplePad, ld2 = (N + 1023) / 1024 * 1024 / 4;
    for (int64_t s : {(int64_t)0, nst / 2, nst - 1})
        for (int sh = 0; sh < 2; ++sh) {
            const int64_t ns = s * kAscStage + 32 * sh;
            EXPECT(ns % 32 == 0 && ns + 32 <= npad, "row fetch N=%lld s=%lld", (long long)N, (long long)s);
            // asc_fetch: int8 = two 16-byte reads at ns and ns + 16, 2-bit = one 8-byte read at ns / 4
            EXPECT(ns + 32 <= ld8 && (ns >> 2) + 8 <= ld2, "row fetch past the pitch N=%lld s=%lld", (long long)N, (long long)s);
            EXPECT(ns % 16 == 0 && ld8 % 16 == 0 && (ns >> 2) % 8 == 0 && ld2 % 8 == 0, "row fetch alignment N=%lld s=%lld", (long long)N, (long long)s);
            EXPECT(s * (kAscStage / 32) + sh < asc_inc_capacity(N), "include word N=%lld s=%lld", (long long)N, (long long)s);
        }
    for (int T : {1, 16, 21})
        for (int tid = 0; tid < kAscStage / 4; ++tid) {
            const int64_t at = (int64_t)asr_col_w(T - 1) * npad + (nst - 1) * kAscStage + 4 * tid + 3;
            EXPECT(at < asc_b_capacity(N, asr_cols(T, 0)) && 4 * tid + 3 < kAscStage, "w column N=%lld T=%d", (long long)N, T);
        }
}

// asg_call_bytes against the allocations of gpca_assoc_score.cpp, one line per dalloc
static void audit_bytes(int64_t N, const std::vector<int>& ms, int T, int Pc) {
    const Call c = plan(ms, T);
    const int L = asr_cols(T, Pc);
    for (int outs = 0; outs < 8; ++outs) {
        const bool stats = outs & 1, ua = outs & 2, info = outs & 4;
        double sum = 0.0;
        sum += 4.0 * (double)asc_b_capacity(N, L);                        // Bt (f32)
        sum += 4.0 * (double)asc_inc_capacity(N);                         // incw (u32)
        sum += 8.0;                                                       // bad (u64)
        sum += 8.0 * (double)asr_dv_capacity(c.listed, L);                // dv
        sum += 4.0 * (double)asr_sums_capacity(c.listed);                 // sums (u32)
        if (stats) sum += 8.0 * (double)asr_stats_capacity(c.listed, T);
        if (ua) sum += 8.0 * (double)asr_ua_capacity(c.listed, T, Pc);
        if (info) sum += 8.0 * (double)asr_info_capacity(c.listed);
        sum += 8.0 * (double)c.listed;                                    // lrows (i64)
        sum += (double)sizeof(AsgStrip) * (double)c.strips.size();        // strips
        sum += 8.0 * (double)c.tri_total * (double)T;                     // phi
        const double got = asg_call_bytes(N, c.listed, (int64_t)c.strips.size(), c.tri_total, T, Pc, stats, ua, info);
        EXPECT(got == sum, "bytes N=%lld T=%d Pc=%d outs=%d: %.0f != %.0f", (long long)N, T, Pc, outs, got, sum);
    }
}

int main() {
    static_assert(sizeof(AsgStrip) == 24, "two i64 and two i32");
    static_assert(kAsgMaxRows == 128 && kAsgStripRows == 32 && kAsgThreads == 256, "a set is one score-scan tile");
    std::mt19937_64 rng(16);
    for (int m = 1; m <= kAsgMaxRows; ++m)
        for (int T : {1, 2, 16}) audit_call({m}, T);
    std::vector<int> all;
    for (int m = 1; m <= kAsgMaxRows; ++m) all.push_back(m);
    audit_call(all, 3);
    audit_call({127, 2, 1, 33, 128, 31, 32, 64, 65}, 16);              // (the GPU test's call)
    for (int t = 0; t < 20; ++t) {
        std::vector<int> ms;
        for (int k = 0; k < 50; ++k) ms.push_back(1 + (int)(rng() % kAsgMaxRows));
        audit_call(ms, 1 + (int)(rng() % 21));
    }
    for (int64_t n_sets : {(int64_t)1000, (int64_t)100000, (int64_t)20000000, (((int64_t)1 << 31) - 1) / 4})
        for (int m : {1, 64, 128})
            for (int T : {1, 21}) audit_large(n_sets, m, T);
    std::vector<int64_t> Ns = {1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1025, 2047, 2048, 2049, 100000, 500000, ((int64_t)1 << 25) + 1,
                               ((int64_t)1 << 30) - 1};
    for (int t = 0; t < 200; ++t) Ns.push_back(1 + (int64_t)(rng() % ((uint64_t)1 << 30)));
    for (int64_t N : Ns) audit_samples(N);
    for (int64_t N : {(int64_t)1, (int64_t)63, (int64_t)2049, (int64_t)100000})
        for (int Pc : {0, 1, 10, 61}) {
            audit_bytes(N, {1}, 1, Pc);
            audit_bytes(N, all, asr_max_traits(Pc), Pc);
            audit_bytes(N, std::vector<int>(1000, 64), 1, Pc);
        }
    printf("assoc_set_plan_audit: %lld checks, %lld failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
