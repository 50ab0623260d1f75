// Extent audit of the cis-QTL call's host arithmetic (genomic_pca_amd/csrc/plan_math.h, the qtl_cis_* and qtl_perm_* functions): over
// (N, n, P, Pc, window, union of the windows, G) at the tile edges and at their limits, every reader and writer of assoc_qtl_cis.hip
// stays inside the buffer gpca_assoc_qtl_cis.cpp allocates for it: the panel, the table, Q, the residuals, the bests of a launch with
// the xb of column 0, the running best and the [G][P] result; the workgroups of k_qtl_perm_panel cover the P + 1 columns once and their
// (column, covariate) pairs fit the workgroup; the launches of a window cover its row blocks once from lo and stay inside the per-row
// buffers of the union; the static LDS of both kernels stays within 64 KiB.  Restates the kernels' index arithmetic on the host;
// includes the header the engine itself uses.
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

// the panel kernel: groups, pairs, the table, Q, the residuals, the panel
static void audit_panel(int64_t N, int64_t n, int64_t P, int Pc, int64_t G) {
    const int grp = qtl_perm_group(Pc);
    const int64_t grid = qtl_perm_grid(P, Pc), npad = asc_npad(N), T = P + 1;
    EXPECT(grp >= 1 && (int64_t)grp * (Pc > 0 ? Pc : 1) <= kQtlPermThreads, "pairs of a group Pc=%d", Pc);
    // thread t of step 1 owns pair (t / Pc, t % Pc): every pair of the group has a thread, and its slot in sc
    EXPECT(Pc == 0 || ((grp - 1) * Pc + Pc - 1 < kQtlPermThreads && (kQtlPermThreads - 1) / Pc >= grp - 1), "threads of step 1 Pc=%d", Pc);
    // the tile of Q: thread k of the fill writes (k / tile, k % tile) for k < Pc * tile; step 1 reads row j up to tile - 1
    EXPECT(Pc == 0 || (Pc - 1) * kQtlPermQPitch + kQtlPermQTile - 1 < kQtlMaxPc * kQtlPermQPitch, "Q tile Pc=%d", Pc);
    EXPECT(grid * grp >= T && (grid - 1) * grp < T && grid >= 1 && grid < ((int64_t)1 << 31), "groups cover the columns P=%lld Pc=%d", (long long)P, Pc);
    // the last column's last sample: the table row P - 1, Q's last covariate, the residual of the last trait, the panel cell
    EXPECT(P == 0 || (P - 1) * n + (n - 1) < qtl_cis_table_capacity(P, n), "table P=%lld n=%lld", (long long)P, (long long)n);
    EXPECT(Pc == 0 || (int64_t)(Pc - 1) * n + (n - 1) < qtl_cis_q_capacity(Pc, n), "Q Pc=%d", Pc);
    EXPECT(qtl_cis_resid_index(G - 1, n, n - 1) < qtl_cis_resid_capacity(G, n), "residuals G=%lld", (long long)G);
    EXPECT(n <= N && qtl_cis_panel_index(P, npad, N - 1) < qtl_cis_panel_capacity(N, P), "panel N=%lld P=%lld", (long long)N, (long long)P);
    // the scan reads the panel as a24's: whole tiles of 64 columns x npad
    EXPECT(qtl_cis_panel_capacity(N, P) == qtl_b_capacity(N, T) && qtl_tile_offset(qtl_tiles(T) - 1, N) + asc_b_capacity(N, kQtlTile) <= qtl_cis_panel_capacity(N, P),
           "panel tiles N=%lld P=%lld", (long long)N, (long long)P);
    EXPECT(P <= kQtlCisMaxPerm && T <= kQtlMaxTraits && qtl_strips(T, kQtlMinTw) <= 65535, "columns P=%lld", (long long)P);
    // the result of the last trait's last permutation
    EXPECT(P == 0 || qtl_cis_result_index(G - 1, P, P - 1) < qtl_cis_result_capacity(G, P), "result G=%lld P=%lld", (long long)G, (long long)P);
    EXPECT(3 * (G - 1) + 2 < qtl_cis_best_capacity(G) && P < qtl_cis_run_capacity(P), "bests G=%lld", (long long)G);
}

// a window [lo, hi) inside the union [ulo, uhi), wrows = the longest window of the call
static void audit_window(int64_t ulo, int64_t lo, int64_t hi, int64_t uhi, int64_t wrows, int64_t P, int64_t forced) {
    const int64_t T = P + 1, rows = uhi - ulo, chunk = qtl_chunk_blocks(T);
    EXPECT(ulo <= lo && lo < hi && hi <= uhi && hi - lo <= wrows, "window [%lld, %lld)", (long long)lo, (long long)hi);
    const int64_t first = asc_row_blocks(hi - lo) < chunk ? asc_row_blocks(hi - lo) : chunk;
    const int tw = qtl_strip_width(first, T, forced);
    EXPECT(tw == qtl_clamp_tw(tw) && qtl_strips(T, tw) <= 65535 && qtl_strips(T, tw) * (tw / kQtlTile) >= qtl_tiles(T), "strips P=%lld", (long long)P);
    int64_t covered = 0, launches = 0;
    for (int64_t r = lo; r < hi; r += chunk * kAscRows) {
        const int64_t re = r + chunk * kAscRows < hi ? r + chunk * kAscRows : hi;
        const int64_t lb = asc_row_blocks(re - r);
        EXPECT((r - lo) % kAscRows == 0 && lb >= 1 && lb <= chunk && lb <= qtl_cis_ws_blocks(wrows, P), "launch r=%lld", (long long)r);
        EXPECT(qtl_wsbest_index(lb - 1, T, T - 1) < qtl_cis_ws_capacity(wrows, P) && lb - 1 < qtl_cis_wsxb_capacity(wrows, P), "bests of a launch P=%lld", (long long)P);
        // the last row the launch reads of the per-row pass over the union; no row below ulo or at or past hi is read
        EXPECT(3 * (re - 1 - ulo) + 2 < asc_sums_capacity(rows) && 4 * (re - 1 - ulo) + 3 < asc_info_capacity(rows) && r - ulo >= 0, "per-row buffers");
        EXPECT((lb - 1) * kAscRows + r < re, "no empty row block");
        covered += lb; ++launches;
        if (launches > 4 && r + 2 * chunk * kAscRows < hi) {
            const int64_t skip = (hi - r) / (chunk * kAscRows) - 2;
            covered += skip * chunk; r += skip * chunk * kAscRows;
        }
    }
    EXPECT(covered == asc_row_blocks(hi - lo), "launches cover the window once [%lld, %lld) P=%lld", (long long)lo, (long long)hi, (long long)P);
    EXPECT(16 * qtl_cis_ws_capacity(wrows, P) <= kQtlBestBytes || qtl_cis_ws_blocks(wrows, P) == 1, "bests workspace");
}

int main() {
    static_assert(qtl_cis_lds_bytes() <= 64 * 1024 && qtl_perm_lds_bytes() <= 64 * 1024, "static LDS of the kernels");
    static_assert(qtl_cis_lds_bytes() == qtl_lds_bytes() - 4 * kAscRows + 32, "k_assoc_qtl's LDS without the hit counts, plus the waves' xb");
    EXPECT(qtl_cis_lds_bytes() == 61472 && qtl_perm_lds_bytes() == 34816 + 8 * 63 * 33, "LDS bytes %lld %lld", (long long)qtl_cis_lds_bytes(), (long long)qtl_perm_lds_bytes());
    std::mt19937_64 rng(25);
    std::vector<int64_t> Ps = {0, 1, 62, 63, 64, 65, 127, 128, 1000, 10000, 65534, 65535};
    std::vector<int64_t> Ns = {3, 17, 63, 64, 65, 255, 256, 257, 1024, 4096, 4097, 100000};
    for (int t = 0; t < 40; ++t) { Ps.push_back((int64_t)(rng() % 65536)); Ns.push_back(3 + (int64_t)(rng() % 300000)); }
    for (int64_t N : Ns)
        for (int64_t P : Ps)
            for (int Pc : {0, 1, 2, 7, 31, 32, 63})
                for (int64_t G : {(int64_t)1, (int64_t)3, (int64_t)20000}) {
                    audit_panel(N, N, P, Pc, G);
                    audit_panel(N, N - (int64_t)(rng() % (uint64_t)(N - 2)), P, Pc, G);
                }
    std::vector<int64_t> Ws = {1, 2, 127, 128, 129, 200, 2048, 8192, 1000003, (int64_t)1 << 31};
    for (int t = 0; t < 40; ++t) Ws.push_back(1 + (int64_t)(rng() % 50000000));
    for (int64_t w : Ws)
        for (int64_t P : Ps)
            for (int64_t forced : {0, 64, 1024}) {
                const int64_t ulo = (int64_t)(rng() % 1000), before = (int64_t)(rng() % 300), after = (int64_t)(rng() % 300);
                audit_window(ulo, ulo + before, ulo + before + w, ulo + before + w + after, w + (int64_t)(rng() % 2 ? 0 : rng() % 100000), P, forced);
            }
    EXPECT(qtl_cis_call_bytes(1024, 1000, 8192, 8192, 64, 10000, 5) >= 4.0 * (double)qtl_cis_panel_capacity(1024, 10000) + 8.0 * 64 * 10000 + 4.0 * 10000 * 1000,
           "call bytes");
    printf("assoc_qtl_cis_plan_audit: %lld checks, %lld failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
