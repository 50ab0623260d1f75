// Extent audit of the QTL scan's host arithmetic (genomic_pca_amd/csrc/plan_math.h, the qtl_* functions): over (rows, N, T, strip width)
// at the tile edges and at their limits, every reader and writer of assoc_qtl.hip stays inside the buffer gpca_assoc_qtl.cpp allocates
// for it, the strips and tiles cover the traits once, the launches of a band cover its row blocks once and stay within the bests'
// workspace, the grid stays within its bounds and the workgroup's LDS within the CU's 160 KiB (and the 64 KiB of a static allocation).
// Restates the kernels' index arithmetic on the host; includes the header the engine itself uses.
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

// the trait axis: tiles, strips, the panel, yy
static void audit_traits(int64_t N, int64_t T, int tw) {
    const int64_t tpad = qtl_tpad(T), ntiles = qtl_tiles(T), strips = qtl_strips(T, tw), npad = asc_npad(N);
    EXPECT(tpad >= T && tpad - T < kQtlTile && tpad == ntiles * kQtlTile, "tpad T=%lld", (long long)T);
    EXPECT(tw == qtl_clamp_tw(tw) && tw % kQtlTile == 0 && tw >= kQtlMinTw && tw <= kQtlMaxTw, "strip width %d", tw);
    const int64_t per = tw / kQtlTile;
    // strip s walks the tiles [s per, (s + 1) per) below ntiles: every tile in exactly one strip, no strip empty
    EXPECT(strips * per >= ntiles && (strips - 1) * per < ntiles && strips >= 1 && strips <= 65535, "strips T=%lld tw=%d", (long long)T, tw);
    // a tile's panel is what k_assoc stages of a 64-column call: asc_fetch_b's last read, from the last tile, stays inside the panel
    EXPECT(kQtlTile == kAscMaxCols && asc_lpad(kQtlTile) == kQtlTile, "a tile is a 64-column call");
    EXPECT(qtl_tile_offset(ntiles - 1, N) + asc_b_capacity(N, kQtlTile) <= qtl_b_capacity(N, T), "panel N=%lld T=%lld", (long long)N, (long long)T);
    EXPECT(qtl_tile_offset(1, N) == kQtlTile * npad && qtl_b_capacity(N, T) == tpad * npad, "tile pitch");
    // the epilogue reads yy of every column of every tile, column < tpad; the bests and the records name columns < T
    EXPECT((ntiles - 1) * kQtlTile + kQtlTile - 1 < qtl_yy_capacity(T), "yy T=%lld", (long long)T);
    EXPECT(T <= kQtlMaxTraits && T - 1 < ((int64_t)1 << 32), "trait index in 32 bits");
}

// the covariate panel of the per-row pass
static void audit_cov(int64_t N, int64_t rows, int Pc) {
    const int L = qtl_cov_cols(Pc);
    EXPECT(L >= 1 && L <= kAscMaxCols && L >= Pc && Pc <= kQtlMaxPc, "covariate columns Pc=%d", Pc);
    EXPECT(qtl_q_capacity(N, Pc) == asc_b_capacity(N, L) && qtl_q_capacity(N, Pc) == (int64_t)asc_lpad(L) * asc_npad(N), "covariate panel Pc=%d", Pc);
    EXPECT((rows - 1) * L + (L - 1) < qtl_xbq_capacity(rows, Pc), "covariate xb rows=%lld", (long long)rows);
}

// the band: launches of at most qtl_chunk_blocks(T) row blocks cover its blocks once; the writers of the last workgroup stay inside
static void audit_band(int64_t rows, int64_t T, int64_t forced, int64_t cap) {
    const int64_t nb = asc_row_blocks(rows), chunk = qtl_wsbest_blocks(rows, T);
    EXPECT(chunk >= 1 && chunk <= nb && chunk <= qtl_chunk_blocks(T), "chunk rows=%lld T=%lld", (long long)rows, (long long)T);
    EXPECT(16 * qtl_wsbest_capacity(rows, T) <= kQtlBestBytes || chunk == 1, "bests workspace rows=%lld T=%lld", (long long)rows, (long long)T);
    const int tw = qtl_strip_width(chunk, T, forced);
    EXPECT(tw == qtl_clamp_tw(tw), "plan's strip width rows=%lld T=%lld forced=%lld", (long long)rows, (long long)T, (long long)forced);
    EXPECT(forced <= 0 || tw == qtl_clamp_tw(forced), "forced width");
    EXPECT(qtl_strips(T, tw) <= 65535 && chunk < ((int64_t)1 << 31), "grid rows=%lld T=%lld", (long long)rows, (long long)T);
    int64_t covered = 0, launches = 0;
    for (int64_t r = 0; r < rows; r += chunk * kAscRows) {
        const int64_t re = r + chunk * kAscRows < rows ? r + chunk * kAscRows : rows;
        const int64_t lb = asc_row_blocks(re - r);
        EXPECT(r % kAscRows == 0 && lb >= 1 && lb <= chunk, "launch rows=%lld r=%lld", (long long)rows, (long long)r);
        // the last workgroup of the launch writes its best of the last trait, and reads / writes the per-row buffers of its last row
        EXPECT(qtl_wsbest_index(lb - 1, T, T - 1) < qtl_wsbest_capacity(rows, T), "bests index rows=%lld T=%lld", (long long)rows, (long long)T);
        EXPECT(3 * (re - 1) + 2 < asc_sums_capacity(rows) && 4 * (re - 1) + 3 < asc_info_capacity(rows) && re - 1 < qtl_hitcount_capacity(rows),
               "per-row buffers rows=%lld", (long long)rows);
        covered += lb; ++launches;
        if (launches > 4 && r + 2 * chunk * kAscRows < rows) {                       // (a long band: jump to its last launches)
            const int64_t skip = (rows - r) / (chunk * kAscRows) - 2;
            covered += skip * chunk; r += skip * chunk * kAscRows;
        }
    }
    EXPECT(covered == nb, "launches cover the row blocks once rows=%lld T=%lld (%lld of %lld)", (long long)rows, (long long)T, (long long)covered, (long long)nb);
    // a record at index < cap: two words of either buffer
    EXPECT(cap == 0 || 2 * (cap - 1) + 1 < qtl_rec_capacity(cap), "records cap=%lld", (long long)cap);
    EXPECT(qtl_call_bytes(1024, rows, T, 10, cap) >= 16.0 * (double)qtl_wsbest_capacity(rows, T) + 12.0 * (double)qtl_rec_capacity(cap), "call bytes");
}

int main() {
    static_assert(qtl_lds_bytes() <= 160 * 1024 && qtl_lds_bytes() <= 64 * 1024, "LDS of a workgroup");
    static_assert(asc_lds_bytes(2, 3) == 2 * kAscRows * kAscGPitch + 2 * 64 * kAscBPitch * 4 + kAscRows * 3 * 4, "k_assoc's stage buffers at 64 columns");
    static_assert(kQtlTile == 64 && kQtlMinTw == 64 && kQtlMaxTw == 1024 && kAscThreads / 64 == 4, "tile, strip widths, four waves");
    EXPECT(qtl_lds_bytes() == 61952, "LDS bytes %lld", (long long)qtl_lds_bytes());
    std::mt19937_64 rng(24);
    const std::vector<int> tws = {64, 128, 256, 512, 1024};
    for (int64_t f : {-5, 0, 1, 63, 64, 65, 127, 128, 129, 1000, 1023, 1024, 1025, 1 << 20}) {
        const int w = qtl_clamp_tw(f);
        EXPECT(w >= 64 && w <= 1024 && (w & (w - 1)) == 0 && (w <= f || w == 64) && (2 * (int64_t)w > f || w == 1024), "clamp %lld -> %d", (long long)f, w);
    }
    std::vector<int64_t> Ts = {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 2051, 8192,
                               20000, 100000, kQtlMaxTraits - 1, kQtlMaxTraits};
    std::vector<int64_t> Ns = {1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 10000, 500000, ((int64_t)1 << 30) - 1};
    std::vector<int64_t> Rs = {1, 127, 128, 129, 300, 2047, 2048, 2049, 4097, 1000003, ((int64_t)1 << 31) - 1, (int64_t)1 << 32};
    for (int t = 0; t < 200; ++t) { Ts.push_back(1 + (int64_t)(rng() % kQtlMaxTraits)); Ns.push_back(1 + (int64_t)(rng() % 200000)); Rs.push_back(1 + (int64_t)(rng() % 30000000)); }
    for (int64_t T : Ts)
        for (int64_t N : Ns)
            for (int tw : tws) audit_traits(N, T, tw);
    for (int64_t N : Ns)
        for (int Pc : {0, 1, 10, 31, 32, 33, 63})
            for (int64_t rows : {(int64_t)1, (int64_t)129, (int64_t)1000003}) audit_cov(N, rows, Pc);
    for (int64_t rows : Rs)
        for (int64_t T : Ts)
            for (int64_t forced : {0, 64, 128, 1024, 5000})
                audit_band(rows, T, forced, (int64_t)(rng() % 3 == 0 ? 0 : 1 + rng() % 100000000));
    printf("assoc_qtl_plan_audit: %lld checks, %lld failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
