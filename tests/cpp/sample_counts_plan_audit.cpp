// Extent audit of the per-sample genotype counts' host arithmetic (genomic_pca_amd/csrc/plan_math.h, the sc_* functions): for every plan
// sc_plan can return over a grid of (rows, N, CUs, forced splits) it walks every workgroup and thread of the launch (sample_counts.hip)
// and holds every fetch inside the row's pitch of both storages (gpca_residency.cpp) with the alignment its vector load needs; counts
// the readers of every (row, sample) of the band (exactly one); holds every slab index of k_sample_counts and k_sc_sum inside the
// buffers gpca_sample_counts.cpp allocates, every slab entry written exactly once and read exactly once; sums the allocations against
// the GPCA_ERR_OOM sum; and bounds the byte counters, the u32 sums and the u64 sums.  Restates the kernels' index arithmetic on the
// host; includes the header the engine itself uses.
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

// one launch: rows kept rows of the band, N samples, the plan p
static void audit_launch(int64_t rows, int64_t N, const ScPlan& p, bool walk_rows) {
    const int64_t npad = sc_npad(N);
    // int8 rows pad to kSamplePad samples, 2-bit rows to 1 024 samples (4 per byte); the pitch is at least that
    const int64_t ld8 = (N + kSamplePad - 1) / kSamplePad * kSamplePad, ld2 = (N + 1023) / 1024 * 1024 / 4;
    EXPECT(npad >= N && npad - N < kScLane && npad % kScLane == 0 && npad <= ld8 && npad <= 4 * ld2, "npad N=%lld", (long long)N);
    EXPECT(p.chunks == sc_chunks(N) && p.chunks * kScChunk >= npad && (p.chunks - 1) * kScChunk < npad, "chunks N=%lld", (long long)N);
    EXPECT(p.splits >= 1 && p.per >= 1 && p.splits <= rows && p.splits * p.per >= rows && (p.splits - 1) * p.per < rows,
           "splits rows=%lld splits=%lld per=%lld", (long long)rows, (long long)p.splits, (long long)p.per);
    EXPECT(sc_grid(p) == p.chunks * p.splits && sc_grid(p) >= 1, "grid");
    const int64_t pcap = sc_part_capacity(p.splits, N), qcap = sc_qpart_capacity(p.splits, N);
    std::vector<uint8_t> sample_readers((size_t)N, 0), pw((size_t)pcap, 0), qw((size_t)qcap, 0);
    std::vector<uint8_t> row_readers;
    if (walk_rows) row_readers.assign((size_t)(rows * N), 0);
    bool inside = true;
    for (int64_t b = 0; b < sc_grid(p); ++b) {
        const int64_t chunk = b % p.chunks, split = b / p.chunks;
        EXPECT(chunk < p.chunks && split < p.splits, "workgroup b=%lld", (long long)b);
        const int64_t ka = split * p.per, kb = ka + p.per < rows ? ka + p.per : rows;
        EXPECT(ka < kb && kb <= rows, "empty split %lld rows=%lld", (long long)split, (long long)rows);
        for (int t = 0; t < kScThreads; ++t) {
            const int64_t n0 = sc_thread_sample(chunk, t);
            if (n0 >= npad) continue;
            // the fetch of a row: 16 bytes (int8) or 4 bytes (2-bit)
            const int64_t o8 = sc_row_offset(false, n0), o2 = sc_row_offset(true, n0);
            EXPECT(o8 >= 0 && o8 + 16 <= ld8 && o8 % 16 == 0, "int8 fetch N=%lld n0=%lld", (long long)N, (long long)n0);
            EXPECT(o2 >= 0 && o2 + 4 <= ld2 && o2 % 4 == 0, "2-bit fetch N=%lld n0=%lld", (long long)N, (long long)n0);
            EXPECT(N - n0 >= 1, "a live thread owns a sample N=%lld n0=%lld", (long long)N, (long long)n0);
            for (int s = 0; s < kScLane; ++s) {
                const int64_t n = n0 + s;
                if (n < N && split == 0 && sample_readers[(size_t)n] < 255) sample_readers[(size_t)n]++;
                if (n < N && walk_rows)
                    for (int64_t k = ka; k < kb; ++k) row_readers[(size_t)(k * N + n)]++;
                // the slab writes: 3 u32 per sample (as 12 aligned uint4 per thread), one u64 per sample (as 8 pairs)
                for (int c = 0; c < 3; ++c) {
                    const int64_t ix = sc_part_index(split, npad, n, c);
                    if (ix < 0 || ix >= pcap) { inside = false; continue; }
                    if (pw[(size_t)ix] < 255) pw[(size_t)ix]++;
                }
                const int64_t iq = sc_qpart_index(split, npad, n);
                if (iq < 0 || iq >= qcap) { inside = false; continue; }
                if (qw[(size_t)iq] < 255) qw[(size_t)iq]++;
            }
            EXPECT(sc_part_index(split, npad, n0, 0) % 4 == 0 && sc_qpart_index(split, npad, n0) % 2 == 0, "slab alignment n0=%lld", (long long)n0);
        }
    }
    EXPECT(inside, "a slab write leaves its buffer rows=%lld N=%lld splits=%lld", (long long)rows, (long long)N, (long long)p.splits);
    bool once = true;
    for (uint8_t v : sample_readers) once = once && v == 1;
    EXPECT(once, "every sample has one owner N=%lld", (long long)N);
    once = true;
    for (uint8_t v : row_readers) once = once && v == 1;
    EXPECT(once, "every (row, sample) read exactly once rows=%lld N=%lld splits=%lld", (long long)rows, (long long)N, (long long)p.splits);
    once = true;
    for (uint8_t v : pw) once = once && v == 1;
    for (uint8_t v : qw) once = once && v == 1;
    EXPECT(once, "every slab entry written exactly once rows=%lld N=%lld splits=%lld", (long long)rows, (long long)N, (long long)p.splits);
    // the sum kernel: thread n < N reads entry (s, n) of every split and writes counts [3 n .. 3 n + 2] and qsum [n]
    bool rin = true;
    for (int64_t n = 0; n < N; n += (N > 4096 ? N / 1024 : 1))
        for (int64_t s = 0; s < p.splits; ++s)
            rin = rin && sc_part_index(s, npad, n, 2) < pcap && sc_qpart_index(s, npad, n) < qcap && sc_part_index(s, npad, n, 0) >= 0;
    EXPECT(rin && 3 * (N - 1) + 2 < sc_counts_capacity(N) && N - 1 < sc_qsum_capacity(N) && sc_q_capacity(rows) >= rows, "sum pass N=%lld", (long long)N);
    // the OOM sum is the allocations
    for (bool hasq : {false, true}) {
        const double sum = 4.0 * (double)pcap + 4.0 * (double)sc_counts_capacity(N) + 8.0 +
                           (hasq ? 8.0 * (double)qcap + 8.0 * (double)sc_qsum_capacity(N) + 4.0 * (double)sc_q_capacity(rows) : 0.0);
        EXPECT(sum == sc_call_bytes(N, rows, p.splits, hasq), "OOM sum N=%lld rows=%lld", (long long)N, (long long)rows);
    }
}

int main() {
    // a byte counter takes one per row for kScFlushRows rows; a u32 sum at most rows < 2^31; a u64 sum at most rows x 2^30 < 2^61
    static_assert(kScFlushRows <= 255 && kScFlushRows % kScUnroll == 0 && kScChunk == kScThreads * kScLane && kScLane == 16, "counters and the thread's 16 samples");
    std::mt19937_64 rng(18);
    std::vector<int64_t> Ns = {1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 10000};
    std::vector<int64_t> Rs = {1, 2, 5, 7, 8, 9, 247, 248, 249, 254, 255, 256, 257, 511, 600, 1000};
    for (int t = 0; t < 6; ++t) { Ns.push_back(1 + (int64_t)(rng() % 5000)); Rs.push_back(1 + (int64_t)(rng() % 1500)); }
    for (int64_t N : Ns)
        for (int64_t rows : Rs) {
            for (int cus : {1, 8, 256, 304}) audit_launch(rows, N, sc_plan(rows, N, cus), N <= 2049 && rows <= 600);
            for (int64_t forced : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)7, rows, rows + 5, (int64_t)1 << 40})
                audit_launch(rows, N, sc_plan(rows, N, 256, forced), N <= 300 && rows <= 600);
        }
    // large shapes: the plan and the extents alone (no walk of the rows), up to the call's limits
    for (int64_t N : {(int64_t)100000, (int64_t)1000003})
        for (int64_t rows : {(int64_t)1, (int64_t)1000000, ((int64_t)1 << 31) - 1}) {
            const ScPlan p = sc_plan(rows, N, 256);
            EXPECT(p.splits * p.per >= rows && (p.splits - 1) * p.per < rows && p.splits >= 1 && sc_grid(p) < ((int64_t)1 << 31), "large plan");
            EXPECT(p.per < ((int64_t)1 << 31) && (double)rows * 1073741824.0 < 18446744073709551616.0, "sums fit");
            EXPECT(sc_part_index(p.splits - 1, sc_npad(N), sc_npad(N) - 1, 2) == sc_part_capacity(p.splits, N) - 1, "last slab entry");
        }
    printf("sample_counts_plan_audit: %lld checks, %lld failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
