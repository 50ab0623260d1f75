// tests/test_cpp_assoc_set.py: formats.hpp's read_set_list, set_weight, set_maf_ok, assoc_set_groups and AssocSetWriter give what their
// twins in genomic_pca_amd/io.py give.  argv: the output prefix, the set list, then the kept IDs.
#include <cmath>
#include <cstdio>

#include "formats.hpp"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const double nan = std::nan("");
    std::vector<std::string> kept;
    for (int i = 3; i < argc; ++i) kept.push_back(argv[i]);
    try {
        for (const gpca_host::VariantSet& s : gpca_host::read_set_list(argv[2], kept)) {
            std::printf("set %s %s %lld", s.name.c_str(), s.chrom.c_str(), (long long)s.pos);
            for (int64_t r : s.rows) std::printf(" %lld", (long long)r);
            std::printf("\n");
        }
    } catch (const std::runtime_error& e) { std::printf("error %s\n", e.what()); }
    for (double f : {0.0, 0.001, 0.01, 0.25, 0.5, 0.75, 0.999, 1.0})
        std::printf("w %.17g %.17g %d %d\n", gpca_host::set_weight(f, true), gpca_host::set_weight(f, false), gpca_host::set_maf_ok(f, 0.01) ? 1 : 0,
                    gpca_host::set_maf_ok(f, 0.5) ? 1 : 0);
    std::printf("w nan %d\n", gpca_host::set_maf_ok(nan, 0.5) ? 1 : 0);
    const std::vector<int64_t> sizes = {128, 1, 64, 128, 128, 3, 100, 7};
    for (int64_t mv : {(int64_t)1 << 26, (int64_t)20000, (int64_t)9000, (int64_t)1})
        for (int64_t T : {1, 3}) {
            std::printf("groups %lld %lld:", (long long)mv, (long long)T);
            for (const auto& g : gpca_host::assoc_set_groups(sizes, T, 2, mv)) std::printf(" %lld-%lld", (long long)g.first, (long long)g.second);
            std::printf("\n");
        }
    gpca_host::ensure_parent(argv[1]);
    gpca_host::AssocSetWriter w(argv[1], "cad");
    gpca_host::VariantSet a, b, c, d;
    a.name = "GENE1"; a.chrom = "1"; a.pos = 1000;
    b.name = "GENE2"; b.chrom = "X"; b.pos = 2500000;
    c.name = "EMPTY"; c.chrom = "2"; c.pos = 7;
    d.name = "ODD"; d.chrom = "3"; d.pos = 9;
    const double r1[10] = {20.0, 0.0123456789, 0.5, 2.5, 1.90625, 123456.789, 31.25, 1.0, 8.0, 0.01};
    const double r2[10] = {3.0, -2.5e-7, 1e-7, -2.5, 1234.5678, 1e-10, 0.0, 0.0, -0.5, nan};
    const double r4[10] = {0.0, nan, nan, nan, nan, nan, nan, 0.0, nan, nan};
    w.add_row(a, 20, r1);
    w.add_row(b, 5, r2);
    w.add_row(c, 0, nullptr);
    w.add_row(d, 2, r4);
    const double r5[10] = {2.0, 1.0, 1.0, 1.0, 0.5, 4.0, 2.0, 2.0, 1.0, 0.1};
    w.add_row(d, 200, nullptr);
    w.add_row(d, 2, r5);
    return 0;
}
