// Dumps what the formats.hpp twins of io.assoc_qtl_bands, io.qtl_best_merge, io.write_qtl_hits and io.write_qtl_best give, for
// tests/test_assoc_qtl_host.py to compare with the Python side.
//   dump_assoc_qtl <out prefix>
#include "formats.hpp"

#include <array>
#include <cmath>
#include <cstdio>

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    for (auto c : {std::array<int64_t, 4>{0, 10, 100, 1000}, {1, 1, 1, 0}, {1000, 8192, 1000, 1 << 20}, {1000000, 8192, 1000, 1 << 20},
                   {1000000, 20000, 500, 1 << 16}, {300, 1, 3, 1}, {5000, 1 << 20, 100000, 1 << 24}, {129, 64, 64, 32}, {100000, 100, 1000, 50}}) {
        std::printf("B %lld %lld %lld %lld", (long long)c[0], (long long)c[1], (long long)c[2], (long long)c[3]);
        for (auto b : gpca_host::assoc_qtl_bands(c[0], c[1], c[2], c[3])) std::printf(" %lld:%lld", (long long)b.first, (long long)b.second);
        std::printf("\n");
    }
    const double nan = std::nan("");
    std::vector<double> b2 = {nan, nan, nan, nan};
    std::vector<int64_t> bw = {-1, -1, -1, -1};
    gpca_host::qtl_best_merge(b2, bw, {0.5, nan, 0.25, 0.0}, {3, -1, 7, 0});
    gpca_host::qtl_best_merge(b2, bw, {0.5, nan, 0.5, 0.0}, {130, -1, 131, 128});
    gpca_host::qtl_best_merge(b2, bw, {0.75, 0.125, nan, 0.0}, {300, 301, -1, 256});
    for (size_t t = 0; t < 4; ++t) std::printf("M %g %lld\n", b2[t], (long long)bw[t]);
    gpca_host::ensure_parent(argv[1]);
    {
        gpca_host::QtlHitsWriter w(argv[1]);
        w.add_hit("1", 100, "rs1", "A", "geneA", 500.0, 0.25, 1.5, 0.5, 3.0, 2.56789012);
        w.add_hit("1", 2500000, "rs2", "G", "geneB", 499.0, 0.123456789, -2.5e-7, 1e-7, -2.5, 1234.5678);
        w.add_hit("X", 7, "rs3", "T", "geneA", 12.0, 0.5, nan, nan, nan, nan);
    }
    {
        gpca_host::QtlBestWriter w(argv[1]);
        w.add_trait("geneA", "1", 100, "rs1", "A", 1.5, 0.5, 3.0, 2.56789012, 1000);
        w.add_none("geneB", 0);
        w.add_trait("geneC", "22", 123456789, "rs9", "C", nan, nan, nan, nan, 7);
    }
    return 0;
}
