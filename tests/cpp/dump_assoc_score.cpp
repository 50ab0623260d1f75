// Dumps what the formats.hpp twins of io.binary_trait, io.assoc_score_groups, io.assoc_score_bands and io.write_assoc_logistic give,
// one line per item, for tests/test_assoc_score_host.py to compare with the Python side.
//   dump_assoc_score <out prefix> <pheno file>...
#include "formats.hpp"

#include <array>
#include <cmath>
#include <cstdio>

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    for (int i = 2; i < argc; ++i) {
        const gpca_host::PhenoTable t = gpca_host::read_pheno(argv[i]);
        std::printf("T");
        for (size_t c = 0; c < t.names.size(); ++c) {
            double shift = -1.0;
            const bool b = gpca_host::binary_trait(t, c, &shift);
            if (b) std::printf(" %s:%g", t.names[c].c_str(), shift); else std::printf(" %s:-", t.names[c].c_str());
        }
        std::printf("\n");
    }
    for (auto tp : {std::pair<int64_t, int64_t>{1, 0}, {21, 0}, {22, 0}, {50, 0}, {5, 10}, {3, 29}, {2, 30}, {7, 61}, {0, 4}}) {
        std::printf("G %lld %lld", (long long)tp.first, (long long)tp.second);
        for (auto g : gpca_host::assoc_score_groups(tp.first, tp.second)) std::printf(" %lld:%lld", (long long)g.first, (long long)g.second);
        std::printf("\n");
    }
    try { gpca_host::assoc_score_groups(1, 62); std::printf("G no error\n"); }
    catch (const std::runtime_error& e) { std::printf("E %s\n", e.what()); }
    for (auto ktp : {std::array<int64_t, 3>{0, 1, 0}, {10, 21, 0}, {200000000, 1, 61}, {3000000, 4, 13}}) {
        std::printf("B");
        for (auto b : gpca_host::assoc_score_bands(ktp[0], ktp[1], ktp[2])) std::printf(" %lld:%lld", (long long)b.first, (long long)b.second);
        std::printf("\n");
    }
    for (auto b : gpca_host::assoc_score_bands(10, 4, 13, 256)) std::printf("b %lld:%lld\n", (long long)b.first, (long long)b.second);
    const double nan = std::nan("");
    gpca_host::ensure_parent(argv[1]);
    gpca_host::AssocLogisticWriter w(argv[1], "cad");
    w.add_row("1", 100, "rs1", "A", 500.0, 0.25, 1.5, 0.5, 3.0, 2.56789012);
    w.add_row("1", 2500000, "rs2", "G", 499.0, 0.123456789, -2.5e-7, 1e-7, -2.5, 1234.5678);
    w.add_row("X", 7, "rs3", "T", 0.0, nan, nan, nan, nan, nan);
    w.add_row("2", 9, "rs4", "C", 12.0, 0.5, 1e10, 123456789.0, 0.0, INFINITY);
    return 0;
}
