// tests/test_fstat_host.py: formats.hpp's fstat_blocks, read_fstats_list, fstat_quad, write_f2_summary and write_fstats give what their
// twins in genomic_pca_amd/io.py give.  argv: the output prefix, the list file, the block spec, the data file:
//     `K P B`, then P group names, then K lines `CHROM POS`, then B x pairs sums and B x pairs counts.
// Prints the blocks of the K SNPs under the spec (or the error) and the parsed list (or the error); writes <prefix>.f2.summary and
// <prefix>.fstats from libgpca.so's gpca_fstat over the sums given.
#include <cstdio>
#include <fstream>

#include "formats.hpp"
#include "gpca.h"

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    const std::string prefix = argv[1];
    std::ifstream in(argv[4]);
    size_t K = 0, P = 0, B = 0;
    in >> K >> P >> B;
    const size_t pairs = P * (P - 1) / 2;
    std::vector<std::string> names(P), chrom(K);
    std::vector<int64_t> pos(K), acc(B * pairs), cnt(B * pairs);
    for (auto& n : names) in >> n;
    for (size_t i = 0; i < K; ++i) in >> chrom[i] >> pos[i];
    for (auto& v : acc) in >> v;
    for (auto& v : cnt) in >> v;
    if (!in) return 3;
    try {
        int32_t nb = 0;
        const std::vector<int32_t> block = gpca_host::fstat_blocks(chrom, pos, argv[3], nb);
        std::printf("blocks %d:", (int)nb);
        for (int32_t b : block) std::printf(" %d", (int)b);
        std::printf("\n");
    } catch (const std::runtime_error& e) { std::printf("error %s\n", e.what()); }
    std::vector<gpca_host::FstatSpec> list;
    try {
        list = gpca_host::read_fstats_list(argv[2], names);
        for (const auto& s : list) {
            int32_t q[4];
            gpca_host::fstat_quad(s, q);
            std::printf("%s", s.kind.c_str());
            for (int32_t g : s.groups) std::printf(" %d", (int)g);
            std::printf(" -> %d %d %d %d\n", (int)q[0], (int)q[1], (int)q[2], (int)q[3]);
        }
    } catch (const std::runtime_error& e) { std::printf("error %s\n", e.what()); return 0; }
    gpca_host::ensure_parent(prefix);
    std::vector<int32_t> quads;
    for (size_t i = 1; i < P; ++i)
        for (size_t j = 0; j < i; ++j) for (size_t k : {j, i, j, i}) quads.push_back((int32_t)k);
    std::vector<double> out(pairs * 6 + 1);
    if (gpca_fstat(acc.data(), cnt.data(), (int32_t)B, (int32_t)P, quads.data(), (int64_t)pairs, out.data()) != GPCA_OK) return 4;
    out.resize(pairs * 6);
    gpca_host::write_f2_summary(prefix, names, out);
    quads.clear();
    for (const auto& s : list) { int32_t q[4]; gpca_host::fstat_quad(s, q); quads.insert(quads.end(), q, q + 4); }
    out.assign(list.size() * 6 + 1, 0.0);
    if (gpca_fstat(acc.data(), cnt.data(), (int32_t)B, (int32_t)P, quads.empty() ? nullptr : quads.data(), (int64_t)list.size(), out.data()) != GPCA_OK) return 5;
    out.resize(list.size() * 6);
    gpca_host::write_fstats(prefix, names, list, out);
    return 0;
}
