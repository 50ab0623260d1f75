// Audit of the band geometry that gpca_grm, gpca_king and gpca_pcrelate share (genomic_pca_amd/csrc/plan_math.h: band_entries,
// band_index, band_tile_count, band_tile_list) for (tile, diagonal) = (64, with), (128, without), (128, with): the GRM, KING and
// PC-Relate kernels.  Exhaustively for every N <= 300 and every band 0 <= row0 < row1 <= N: the tile list has band_tile_count entries,
// every band entry (a, b) is owned by exactly one (tile, 32 x 32 sub-tile not skipped above the diagonal, accumulator element, lane
// half), the indices of the owned entries are a permutation of [0, band_entries), and no owned element lies outside the band.  The
// work is split by what each property depends on: which (a, b) a tile's lanes own depends on N alone (the a < N, b < N guards), so it
// is walked once per N over all tiles; a band then owns the rows [row0, row1) of that map provided each of its rows lies in a listed
// tile row, which is checked per band with the list itself; the index walk depends on row0 alone, and a band is a prefix of it that
// ends at band_entries.  Then the random large-N sweep of bands at and off the tile edges.
// The kernels' accumulator row map is restated here by hand (row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), column = lane & 31), not
// included from the kernels' header.
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

struct Tile { int x, y; };
struct Geometry { int tile; bool diag; };
static const Geometry kGeometries[] = {{kGrmTile, true}, {kKingTile, false}, {kPcrTile, true}};
constexpr int64_t kMaxN = 300;

static bool in_triangle(int64_t a, int64_t b, bool diag) { return b >= 0 && (diag ? b <= a : b < a); }

// every entry of the triangle of N samples has exactly one owner among the lanes of all tiles, and the lanes own nothing else
static void audit_owners(const Geometry& g, int64_t N) {
    const int64_t T = (N + g.tile - 1) / g.tile, sub = g.tile / 32;
    std::vector<int> owners((size_t)(N * N), 0);
    for (int64_t ta = 0; ta < T; ++ta)
        for (int64_t tb = 0; tb <= ta; ++tb)
            for (int64_t wa = 0; wa < sub; ++wa)
                for (int64_t wb = 0; wb < sub; ++wb) {
                    if (ta == tb && wb > wa) continue;                        // the sub-tile above the diagonal of a diagonal tile
                    for (int lane = 0; lane < 64; ++lane)
                        for (int reg = 0; reg < 16; ++reg) {
                            const int64_t a = ta * g.tile + 32 * wa + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
                            const int64_t b = tb * g.tile + 32 * wb + (lane & 31);
                            if (b >= N || a >= N || !(g.diag ? b <= a : b < a)) continue;     // the kernels' guards
                            EXPECT(in_triangle(a, b, g.diag) && a < N, "tile %d N=%lld: owned (%lld, %lld) outside", g.tile, (long long)N, (long long)a, (long long)b);
                            ++owners[(size_t)(a * N + b)];
                        }
                }
    for (int64_t a = 0; a < N; ++a)
        for (int64_t b = 0; b < N; ++b)
            EXPECT(owners[(size_t)(a * N + b)] == (in_triangle(a, b, g.diag) ? 1 : 0), "tile %d diag %d N=%lld: (%lld, %lld) has %d owners", g.tile,
                   (int)g.diag, (long long)N, (long long)a, (long long)b, owners[(size_t)(a * N + b)]);
}

// the tile list of a band: its count, its order, and that it holds the tile row of every band row
static void audit_tiles(const Geometry& g, int64_t row0, int64_t row1) {
    std::vector<Tile> tiles;
    band_tile_list(row0, row1, g.tile, tiles);
    const int64_t t0 = row0 / g.tile, t1 = (row1 + g.tile - 1) / g.tile;
    EXPECT((int64_t)tiles.size() == band_tile_count(row0, row1, g.tile), "tile %d band %lld:%lld: %zu tiles listed", g.tile, (long long)row0, (long long)row1, tiles.size());
    size_t i = 0;
    for (int64_t ta = t0; ta < t1; ++ta)
        for (int64_t tb = 0; tb <= ta; ++tb, ++i)
            EXPECT(i < tiles.size() && tiles[i].x == ta && tiles[i].y == tb, "tile %d band %lld:%lld: entry %zu", g.tile, (long long)row0, (long long)row1, i);
    EXPECT(i == tiles.size(), "tile %d band %lld:%lld: listed past the band", g.tile, (long long)row0, (long long)row1);
    for (int64_t a = row0; a < row1; ++a)
        EXPECT(a / g.tile >= t0 && a / g.tile < t1, "tile %d band %lld:%lld: row %lld in no listed tile", g.tile, (long long)row0, (long long)row1, (long long)a);
}

// the entries of the rows from row0 on, in row-major order, have the indices 0, 1, 2, ...; a band ends at band_entries
static void audit_index_walk(bool diag, int64_t row0, int64_t nmax) {
    int64_t next = 0;
    for (int64_t a = row0; a < nmax; ++a) {
        for (int64_t b = 0; in_triangle(a, b, diag); ++b, ++next)
            EXPECT(band_index(row0, a, b, diag) == next, "diag %d row0=%lld: index of (%lld, %lld)", (int)diag, (long long)row0, (long long)a, (long long)b);
        EXPECT(band_entries(row0, a + 1, diag) == next, "diag %d: entries of %lld:%lld", (int)diag, (long long)row0, (long long)(a + 1));
    }
}

// a band of any size: entries, the tile count (the list itself would hold up to 3e7 tiles), and the tile and sub-tile that own some of
// its entries
static void audit_band(const Geometry& g, int64_t N, int64_t row0, int64_t row1) {
    const int64_t E = band_entries(row0, row1, g.diag);
    if (E > 0) {
        const int64_t af = g.diag ? row0 : std::max<int64_t>(row0, 1), al = row1 - 1;       // the first and the last row that hold an entry
        EXPECT(band_index(row0, af, 0, g.diag) == 0 && band_index(row0, al, g.diag ? al : al - 1, g.diag) == E - 1,
               "band ends row0=%lld row1=%lld", (long long)row0, (long long)row1);
    }
    const int64_t t0 = row0 / g.tile, t1 = (row1 + g.tile - 1) / g.tile;
    int64_t nt = 0;
    for (int64_t ta = t0; ta < t1; ++ta) nt += ta + 1;
    EXPECT(nt == band_tile_count(row0, row1, g.tile), "tiles row0=%lld row1=%lld", (long long)row0, (long long)row1);
    for (int64_t a : {row0, (row0 + row1) / 2, row1 - 1})
        for (int64_t b : {(int64_t)0, a / 2, g.diag ? a : a - 1}) {
            if (!in_triangle(a, b, g.diag)) continue;
            const int64_t ta = a / g.tile, tb = b / g.tile;
            EXPECT(ta >= t0 && ta < t1 && tb <= ta, "entry (%lld, %lld) in no tile", (long long)a, (long long)b);
            // the wave of the tile that holds it: sub-tile (wa, wb), skipped only above the diagonal of a diagonal tile
            const int64_t wa = (a % g.tile) / 32, wb = (b % g.tile) / 32;
            EXPECT(!(ta == tb && wb > wa), "entry (%lld, %lld) in a skipped sub-tile", (long long)a, (long long)b);
            const int64_t ix = band_index(row0, a, b, g.diag);
            EXPECT(ix >= 0 && ix < E, "index (%lld, %lld)", (long long)a, (long long)b);
        }
    EXPECT(row1 <= N, "band inside the samples");
}

int main() {
    // the row map covers the 32 rows of a sub-tile once per lane half pair
    {
        int seen[32] = {0};
        for (int h = 0; h < 2; ++h)
            for (int reg = 0; reg < 16; ++reg) ++seen[(reg & 3) + 8 * (reg >> 2) + 4 * h];
        for (int r = 0; r < 32; ++r) EXPECT(seen[r] == 1, "row map: row %d written %d times", r, seen[r]);
    }
    for (const Geometry& g : kGeometries) {
        for (int64_t N = 1; N <= kMaxN; ++N) audit_owners(g, N);
        for (int64_t row0 = 0; row0 < kMaxN; ++row0)
            for (int64_t row1 = row0 + 1; row1 <= kMaxN; ++row1) audit_tiles(g, row0, row1);
    }
    for (bool diag : {false, true})
        for (int64_t row0 = 0; row0 < kMaxN; ++row0) audit_index_walk(diag, row0, kMaxN);

    std::mt19937_64 rng(11);
    std::vector<int64_t> Ns = {1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2085, 10000, 50000, 500000};
    for (int t = 0; t < 300; ++t) Ns.push_back(1 + (int64_t)(rng() % 200000));
    for (const Geometry& g : kGeometries)
        for (int64_t N : Ns)
            for (int t = 0; t < 40; ++t) {
                int64_t r0 = t == 0 ? 0 : (int64_t)(rng() % (uint64_t)N), r1 = t == 0 ? N : r0 + 1 + (int64_t)(rng() % (uint64_t)(N - r0));
                for (int64_t e0 : {r0, r0 / g.tile * g.tile}) audit_band(g, N, e0, r1);
                audit_band(g, N, r0, r0 + 1);
            }
    printf("band_plan_audit: %lld checks, %lld failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
