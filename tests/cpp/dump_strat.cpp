// tests/test_fst_host.py: formats.hpp's read_within, align_within, group_count_bands, FrqStratWriter, write_fst_summary and FstVarWriter
// give what their twins in genomic_pca_amd/io.py give.  argv: the output prefix, the within file, the data file:
//     `M P S`, then P group names, then M lines `CHROM POS ID A1` + 3 P counts, then S lines `FID IID`.
// Writes <prefix>.frq.strat, <prefix>_h.fst.summary / .fst.var (Hudson) and <prefix>_w.fst.summary / .fst.var (Weir-Cockerham, r = 2 per
// pair, all groups jointly in the last line) through libgpca.so's host functions, in two bands; prints the table and the labels.
#include <cstdio>
#include <fstream>

#include "formats.hpp"
#include "gpca.h"

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const std::string prefix = argv[1];
    std::ifstream in(argv[3]);
    size_t M = 0, P = 0, S = 0;
    in >> M >> P >> S;
    std::vector<std::string> names(P), chrom(M), id(M), a1(M), fid(S), iid(S);
    std::vector<int64_t> pos(M);
    std::vector<uint32_t> counts(M * P * 3);
    for (auto& n : names) in >> n;
    for (size_t i = 0; i < M; ++i) {
        in >> chrom[i] >> pos[i] >> id[i] >> a1[i];
        for (size_t k = 0; k < 3 * P; ++k) in >> counts[i * 3 * P + k];
    }
    for (size_t s = 0; s < S; ++s) in >> fid[s] >> iid[s];
    if (!in) return 3;
    try {
        const gpca_host::WithinTable t = gpca_host::read_within(argv[2]);
        std::printf("names");
        for (const std::string& n : t.names) std::printf(" %s", n.c_str());
        std::printf("\nlabels");
        for (int32_t g : gpca_host::align_within(t, fid, iid)) std::printf(" %d", (int)g);
        std::printf("\n");
    } catch (const std::runtime_error& e) { std::printf("error %s\n", e.what()); }
    for (int64_t mv : {(int64_t)1 << 26, (int64_t)1000, (int64_t)1})
        for (int64_t p : {1, 3, 64}) {
            std::printf("bands %lld %lld:", (long long)mv, (long long)p);
            for (const auto& b : gpca_host::group_count_bands(1000, p, mv)) std::printf(" %lld-%lld", (long long)b.first, (long long)b.second);
            std::printf("\n");
        }
    gpca_host::ensure_parent(prefix);
    const size_t pairs = P * (P - 1) / 2, cut = M / 2;
    std::vector<double> hud(pairs * 3, 0.0), wcp(pairs * 3, 0.0), wcj(3, 0.0);
    gpca_host::FrqStratWriter wf(prefix + ".frq.strat", names, gpca_hwe_chi_squared_p_value);
    gpca_host::FstVarWriter wh(prefix + "_h", false, names), ww(prefix + "_w", true, names);
    for (int band = 0; band < 2; ++band) {
        const size_t r0 = band ? cut : 0, r1 = band ? M : cut, nr = r1 - r0;
        const uint32_t* c = counts.data() + r0 * P * 3;
        std::vector<double> num(nr * pairs + 1), den(nr * pairs + 1), abc(nr * 3 + 1), hv(nr * pairs * 2 + 1), wv(nr * pairs * 3 + 1);
        if (gpca_fst_hudson(c, (int64_t)nr, (int32_t)P, num.data(), den.data(), hud.data()) != GPCA_OK) return 4;
        for (size_t k = 0; k < nr * pairs; ++k) { hv[2 * k] = num[k]; hv[2 * k + 1] = den[k]; }
        size_t q = 0;
        for (size_t i = 1; i < P; ++i)
            for (size_t j = 0; j < i; ++j, ++q) {
                std::vector<uint8_t> use(P, 0);
                use[i] = use[j] = 1;
                if (gpca_fst_wc(c, (int64_t)nr, (int32_t)P, use.data(), abc.data(), &wcp[3 * q]) != GPCA_OK) return 5;
                for (size_t r = 0; r < nr; ++r) for (size_t k = 0; k < 3; ++k) wv[(r * pairs + q) * 3 + k] = abc[3 * r + k];
            }
        if (P > 2 && gpca_fst_wc(c, (int64_t)nr, (int32_t)P, nullptr, nullptr, wcj.data()) != GPCA_OK) return 6;
        for (size_t r = 0; r < nr; ++r) {
            wf.add_row(chrom[r0 + r], pos[r0 + r], id[r0 + r], a1[r0 + r], c + r * P * 3);
            wh.add_row(chrom[r0 + r], pos[r0 + r], id[r0 + r], &hv[r * pairs * 2]);
            ww.add_row(chrom[r0 + r], pos[r0 + r], id[r0 + r], &wv[r * pairs * 3]);
        }
    }
    gpca_host::write_fst_summary(prefix + "_h", false, names, hud);
    if (P > 2) wcp.insert(wcp.end(), wcj.begin(), wcj.end());
    gpca_host::write_fst_summary(prefix + "_w", true, names, wcp);
    return 0;
}
