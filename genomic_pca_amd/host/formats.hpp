// Host-side file formats either side of the hot path, C++ twin of genomic_pca_amd/io.py:
// PLINK .bed/.bim/.fam, LD-block files, sample keep lists, a VCF genotype reader (plain or gzip/bgzf) and the TSV writers.
// Text parsing stays on the host; genotype bytes go to the GPU untouched (the memory-mapped 2-bit .bed payload, or int8
// dosages) and are decoded / QC'd there.
//
// Reference behaviour restated (file:line):
//   * BED: 3-byte magic 6c 1b 01 (SNP-major), ceil(N/4) bytes per SNP, 2 bits per sample LSB-first (tests/disk.py:89-135);
//     .bim chrom/sid/bp columns, .fam iid column (prepare.rs:940-970 via bed_reader).
//   * LD blocks: prepare.rs:1565-1616 (skip '#', "chr\t", "chromosome\t" headers; tag "chr:start-end"; chromosome names
//     lower-cased with leading "chr" stripped); SNP -> first matching block (prepare.rs:1447-1463).
//   * VCF: biallelic single-base REF/ALT only (vcf.rs:109-121); GT "a/b" or "a|b" with alleles 0/1, anything else drops
//     the variant (vcf.rs:52-63, 153-240); MAF filter default 0.01 (vcf.rs:244-266); id chr:pos:ref:alt.
//   * writers: main.rs:696-839 ("{:.6}" fixed formatting, the exact headers and file suffixes).
#ifndef GPCA_HOST_FORMATS_HPP
#define GPCA_HOST_FORMATS_HPP

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdlib>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

namespace gpca_host {

inline std::vector<std::string> split_ws(const std::string& s) {
    std::vector<std::string> out;
    size_t i = 0;
    while (i < s.size()) {
        while (i < s.size() && std::isspace((unsigned char)s[i])) ++i;
        size_t j = i;
        while (j < s.size() && !std::isspace((unsigned char)s[j])) ++j;
        if (j > i) out.emplace_back(s, i, j - i);
        i = j;
    }
    return out;
}

inline bool ends_with(const std::string& s, const std::string& suf) {
    return s.size() >= suf.size() && s.compare(s.size() - suf.size(), suf.size(), suf) == 0;
}

// ---------------------------------------------------------------------------------------------- PLINK
struct PlinkFileset {
    const uint8_t* bed_rows = nullptr;   // [M][ceil(N/4)]: the memory-mapped .bed payload (after the 3-byte magic)
    int64_t n_snps = 0, n_samples = 0, bytes_per_row = 0;
    std::vector<std::string> sample_ids, variant_ids, chromosomes;
    std::vector<int64_t> positions;
    std::vector<std::string> allele1, allele2;   // .bim columns 5 / 6: A1 (the allele the dosages count), A2
    std::vector<std::string> family_ids;         // .fam FID
    void* map_base = nullptr; size_t map_len = 0;
    PlinkFileset() = default;
    PlinkFileset(const PlinkFileset&) = delete;
    PlinkFileset& operator=(const PlinkFileset&) = delete;
    ~PlinkFileset() { if (map_base) munmap(map_base, map_len); }
};

inline std::string strip_plink_ext(const std::string& p) {
    for (const char* e : {".bed", ".bim", ".fam"}) if (ends_with(p, e)) return p.substr(0, p.size() - 4);
    return p;
}

inline void read_plink(const std::string& bed_path, PlinkFileset& fs) {
    const std::string prefix = strip_plink_ext(bed_path);
    std::string line;
    {
        std::ifstream f(prefix + ".fam");
        if (!f) throw std::runtime_error("cannot open " + prefix + ".fam");
        while (std::getline(f, line)) {
            const auto p = split_ws(line);
            if (!p.empty()) { fs.sample_ids.push_back(p.size() > 1 ? p[1] : p[0]); fs.family_ids.push_back(p[0]); }
        }
    }
    {
        std::ifstream f(prefix + ".bim");
        if (!f) throw std::runtime_error("cannot open " + prefix + ".bim");
        while (std::getline(f, line)) {
            const auto p = split_ws(line);
            if (p.size() >= 4) {
                fs.chromosomes.push_back(p[0]); fs.variant_ids.push_back(p[1]); fs.positions.push_back(std::stoll(p[3]));
                fs.allele1.push_back(p.size() > 4 ? p[4] : "."); fs.allele2.push_back(p.size() > 5 ? p[5] : ".");
            }
        }
    }
    fs.n_samples = (int64_t)fs.sample_ids.size(); fs.n_snps = (int64_t)fs.variant_ids.size();
    fs.bytes_per_row = (fs.n_samples + 3) / 4;
    const std::string bed = prefix + ".bed";
    const int fd = open(bed.c_str(), O_RDONLY);
    if (fd < 0) throw std::runtime_error("cannot open " + bed);
    struct stat sb;
    if (fstat(fd, &sb) != 0) { close(fd); throw std::runtime_error("cannot stat " + bed); }
    unsigned char magic[3] = {0, 0, 0};
    if (pread(fd, magic, 3, 0) != 3 || magic[0] != 0x6c || magic[1] != 0x1b || magic[2] != 0x01) {
        close(fd); throw std::runtime_error(bed + ": not a SNP-major PLINK .bed");
    }
    if ((int64_t)sb.st_size != 3 + fs.n_snps * fs.bytes_per_row) {
        close(fd);
        throw std::runtime_error(bed + ": size " + std::to_string((long long)sb.st_size) + " does not match " + std::to_string(fs.n_snps) + " SNPs x " +
                                 std::to_string(fs.n_samples) + " samples");
    }
    fs.map_len = (size_t)sb.st_size;
    fs.map_base = mmap(nullptr, fs.map_len, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (fs.map_base == MAP_FAILED) { fs.map_base = nullptr; throw std::runtime_error("cannot mmap " + bed); }
    fs.bed_rows = static_cast<const uint8_t*>(fs.map_base) + 3;
}

// ---------------------------------------------------------------------------------------------- LD blocks
inline std::string normalize_chromosome_name(std::string name) {   // prepare.rs:1610-1616
    std::transform(name.begin(), name.end(), name.begin(), [](unsigned char c) { return (char)std::tolower(c); });
    while (name.compare(0, 3, "chr") == 0) name = name.substr(3);
    return name;
}

struct LdBlock { std::string chrom; int64_t start, end; std::string tag; };

inline std::string trim(const std::string& s) {
    size_t a = 0, b = s.size();
    while (a < b && std::isspace((unsigned char)s[a])) ++a;
    while (b > a && std::isspace((unsigned char)s[b - 1])) --b;
    return s.substr(a, b - a);
}

inline std::vector<LdBlock> parse_ld_block_file(const std::string& path) {   // prepare.rs:1565-1607
    std::ifstream f(path);
    if (!f) throw std::runtime_error("cannot open LD block file " + path);
    std::vector<LdBlock> blocks;
    std::string line;
    while (std::getline(f, line)) {
        const std::string t = trim(line);
        if (t.empty() || t[0] == '#' || t.compare(0, 4, "chr\t") == 0 || t.compare(0, 11, "chromosome\t") == 0) continue;
        const auto p = split_ws(t);
        if (p.size() < 3) continue;
        LdBlock b;
        b.chrom = normalize_chromosome_name(p[0]); b.start = std::stoll(p[1]); b.end = std::stoll(p[2]);
        b.tag = b.chrom + ":" + std::to_string(b.start) + "-" + std::to_string(b.end);
        blocks.push_back(b);
    }
    return blocks;
}

// prepare.rs:1424-1563: every QC-passing SNP goes to the FIRST block (file order) that contains it.  Returns the keep mask
// restricted to SNPs inside some block and the blocks' original row lists, sorted by tag.
inline std::vector<std::pair<std::string, std::vector<int64_t>>> map_snps_to_ld_blocks(
    const std::vector<LdBlock>& blocks, const std::vector<std::string>& chromosomes, const std::vector<int64_t>& positions,
    const std::vector<uint8_t>& qc_keep, std::vector<uint8_t>& keep_out) {
    const size_t M = positions.size();
    std::vector<std::string> norm(M);
    for (size_t i = 0; i < M; ++i) norm[i] = normalize_chromosome_name(chromosomes[i]);
    // blocks per chromosome, in file order
    std::map<std::string, std::vector<size_t>> by_chrom;
    for (size_t b = 0; b < blocks.size(); ++b) by_chrom[blocks[b].chrom].push_back(b);
    std::vector<int64_t> assigned(M, -1);
    for (size_t i = 0; i < M; ++i) {
        if (!qc_keep[i]) continue;
        const auto it = by_chrom.find(norm[i]);
        if (it == by_chrom.end()) continue;
        for (size_t b : it->second)
            if (positions[i] >= blocks[b].start && positions[i] <= blocks[b].end) { assigned[i] = (int64_t)b; break; }
    }
    keep_out.assign(M, 0);
    std::map<std::string, std::vector<int64_t>> by_tag;
    for (size_t i = 0; i < M; ++i)
        if (assigned[i] >= 0) { keep_out[i] = 1; by_tag[blocks[(size_t)assigned[i]].tag].push_back((int64_t)i); }
    std::vector<std::pair<std::string, std::vector<int64_t>>> out(by_tag.begin(), by_tag.end());   // std::map: sorted by tag, rows ascending
    return out;
}

inline std::vector<std::string> read_sample_keep_file(const std::string& path) {
    std::ifstream f(path);
    if (!f) throw std::runtime_error("cannot open sample keep file " + path);
    std::vector<std::string> ids;
    std::string line;
    while (std::getline(f, line)) { const auto p = split_ws(line); if (!p.empty()) ids.push_back(p[0]); }
    return ids;
}

// ---------------------------------------------------------------------------------------------- VCF
// A line reader over zlib's gzFile: reads plain text, gzip and bgzf (concatenated gzip members) alike.
class LineReader {
public:
    explicit LineReader(const std::string& path) : gz_(gzopen(path.c_str(), "rb")) {
        if (!gz_) throw std::runtime_error("cannot open " + path);
        gzbuffer(gz_, 1 << 20);
        buf_.resize(1 << 20);
    }
    ~LineReader() { if (gz_) gzclose(gz_); }
    LineReader(const LineReader&) = delete;
    LineReader& operator=(const LineReader&) = delete;
    bool next(std::string& line) {
        line.clear();
        for (;;) {
            if (pos_ == len_) {
                const int n = gzread(gz_, buf_.data(), (unsigned)buf_.size());
                if (n < 0) throw std::runtime_error("read error in compressed stream");
                if (n == 0) return !line.empty();
                pos_ = 0; len_ = (size_t)n;
            }
            const char* p = static_cast<const char*>(std::memchr(buf_.data() + pos_, '\n', len_ - pos_));
            if (p) { line.append(buf_.data() + pos_, (size_t)(p - (buf_.data() + pos_))); pos_ = (size_t)(p - buf_.data()) + 1; break; }
            line.append(buf_.data() + pos_, len_ - pos_);
            pos_ = len_;
        }
        while (!line.empty() && (line.back() == '\r' || line.back() == '\n')) line.pop_back();
        return true;
    }
private:
    gzFile gz_;
    std::vector<char> buf_;
    size_t pos_ = 0, len_ = 0;
};

struct VcfData {
    std::vector<std::string> samples, variant_ids;
    std::vector<int8_t> dosages;      // [variants][samples], SNP-major
};

// the genotype of one sample field whose GT sits at FORMAT position gi: exactly 3 bytes a/b or a|b, alleles 0/1 (vcf.rs:52-63)
inline int gt_dosage(const char* f, const char* fend, int gi) {
    for (int c = 0; c < gi; ++c) {
        const char* q = static_cast<const char*>(std::memchr(f, ':', (size_t)(fend - f)));
        if (!q) return -1;
        f = q + 1;
    }
    const char* q = static_cast<const char*>(std::memchr(f, ':', (size_t)(fend - f)));
    const char* e = q ? q : fend;
    if (e - f != 3 || (f[1] != '/' && f[1] != '|') || (f[0] != '0' && f[0] != '1') || (f[2] != '0' && f[2] != '1')) return -1;
    return (f[0] - '0') + (f[2] - '0');
}

// vcf.rs:65-286: appends the variants of one file that pass the rules; the first file defines the sample list
inline void read_vcf(const std::string& path, double maf_threshold, VcfData& out, bool first_file) {
    LineReader rd(path);
    std::string line;
    std::vector<std::string> samples;
    std::vector<int8_t> d;
    while (rd.next(line)) {
        if (line.compare(0, 2, "##") == 0) continue;
        if (line.compare(0, 6, "#CHROM") == 0) {
            size_t pos = 0; int col = 0;
            while (pos <= line.size()) {
                const size_t tab = line.find('\t', pos);
                const size_t e = tab == std::string::npos ? line.size() : tab;
                if (col >= 9) samples.emplace_back(line, pos, e - pos);
                ++col;
                if (tab == std::string::npos) break;
                pos = tab + 1;
            }
            if (samples.empty()) throw std::runtime_error("VCF header from " + path + " contains no samples.");      // vcf.rs:31-36
            if (first_file) out.samples = samples;
            else if (samples != out.samples) throw std::runtime_error("Sample mismatch between VCF files: " + path);   // vcf.rs:78-95
            d.resize(samples.size());
            continue;
        }
        if (samples.empty()) continue;
        // the first nine columns
        size_t col_start[10]; size_t pos = 0; int ncol = 0;
        while (ncol < 10) {
            col_start[ncol++] = pos;
            const size_t tab = line.find('\t', pos);
            if (tab == std::string::npos) break;
            pos = tab + 1;
        }
        if (ncol < 10) continue;
        auto col = [&](int c) { return std::string(line, col_start[c], col_start[c + 1] - col_start[c] - 1); };
        const std::string ref = col(3), alt = col(4);
        if (ref.size() != 1 || alt.size() != 1 || alt == ",") continue;                                                // vcf.rs:109-121
        const std::string fmt = col(8);
        int gi = -1, idx = 0;
        for (size_t a = 0; a <= fmt.size();) {
            const size_t c = fmt.find(':', a);
            const size_t e = c == std::string::npos ? fmt.size() : c;
            if (fmt.compare(a, e - a, "GT") == 0 && gi < 0) gi = idx;
            ++idx;
            if (c == std::string::npos) break;
            a = c + 1;
        }
        if (gi < 0) continue;
        const size_t ns = samples.size();
        const char* p = line.data() + col_start[9];
        const char* end = line.data() + line.size();
        bool ok = true;
        int64_t sum = 0;
        size_t si = 0;
        while (ok) {
            const char* t = static_cast<const char*>(std::memchr(p, '\t', (size_t)(end - p)));
            const char* fe = t ? t : end;
            if (si >= ns) { ok = false; break; }
            const int v = gt_dosage(p, fe, gi);
            if (v < 0) { ok = false; break; }                                                                            // any bad GT drops the variant
            d[si++] = (int8_t)v; sum += v;
            if (!t) break;
            p = t + 1;
        }
        if (!ok || si != ns) continue;
        const double af = (double)sum / (2.0 * (double)ns);
        if (std::min(af, 1.0 - af) < maf_threshold) continue;                                                           // vcf.rs:244-266
        out.variant_ids.push_back(col(0) + ":" + col(1) + ":" + ref + ":" + alt);
        out.dosages.insert(out.dosages.end(), d.begin(), d.end());
    }
    if (first_file && out.samples.empty() && !samples.empty()) out.samples = samples;
}

// ---------------------------------------------------------------------------------------------- writers
inline void ensure_parent(const std::string& prefix) {   // main.rs:372-377
    const size_t s = prefix.find_last_of('/');
    if (s == std::string::npos || s == 0) return;
    const std::string dir = prefix.substr(0, s);
    std::string cur;
    size_t pos = 0;
    while (pos <= dir.size()) {
        const size_t n = dir.find('/', pos);
        cur = dir.substr(0, n == std::string::npos ? dir.size() : n);
        if (!cur.empty()) mkdir(cur.c_str(), 0777);
        if (n == std::string::npos) break;
        pos = n + 1;
    }
}

struct OutFile {
    FILE* f;
    explicit OutFile(const std::string& path) : f(std::fopen(path.c_str(), "w")) {
        if (!f) throw std::runtime_error("cannot create " + path);
        std::setvbuf(f, nullptr, _IOFBF, 1 << 20);
    }
    ~OutFile() { if (f) std::fclose(f); }
};

// main.rs:696-762: header SampleID\tPC1..; "{:.6}".  suffix = "vcf.pca.tsv" or "eigensnp.pca.tsv"; pcs is [rows][k]
template <typename T>
inline void write_principal_components(const std::string& prefix, const std::string& suffix, const std::vector<std::string>& sample_names,
                                       const T* pcs, int64_t rows, int k) {
    if (k == 0) return;
    OutFile o(prefix + "." + suffix);
    std::fputs("SampleID", o.f);
    for (int c = 1; c <= k; ++c) std::fprintf(o.f, "\tPC%d", c);
    std::fputc('\n', o.f);
    for (size_t i = 0; i < sample_names.size(); ++i) {
        std::fputs(sample_names[i].c_str(), o.f);
        for (int c = 0; c < k; ++c) {
            if ((int64_t)i < rows) std::fprintf(o.f, "\t%.6f", (double)pcs[i * (size_t)k + (size_t)c]);
            else std::fputs("\tNA", o.f);
        }
        std::fputc('\n', o.f);
    }
}

inline void write_eigenvalues(const std::string& prefix, const std::vector<double>& ev) {   // main.rs:765-784: header even when empty
    OutFile o(prefix + ".eigenvalues.tsv");
    std::fputs("PC\tEigenvalue\n", o.f);
    for (size_t i = 0; i < ev.size(); ++i) std::fprintf(o.f, "%zu\t%.6f\n", i + 1, ev[i]);
}

inline void write_loadings(const std::string& prefix, const std::vector<std::string>& variant_ids, const std::vector<std::string>& chroms,
                           const std::vector<int64_t>& positions, const float* loadings, int64_t rows, int k) {   // main.rs:787-839
    if (k == 0) return;
    if (!variant_ids.empty() && !(variant_ids.size() == chroms.size() && chroms.size() == positions.size() && (int64_t)positions.size() == rows))
        throw std::runtime_error("Mismatch in lengths of variant metadata and loadings matrix rows.");   // main.rs:817-824
    OutFile o(prefix + ".eigensnp.loadings.tsv");
    std::fputs("VariantID\tChrom\tPos", o.f);
    for (int c = 1; c <= k; ++c) std::fprintf(o.f, "\tPC%d_loading", c);
    std::fputc('\n', o.f);
    for (size_t i = 0; i < variant_ids.size(); ++i) {
        std::fprintf(o.f, "%s\t%s\t%lld", variant_ids[i].c_str(), chroms[i].c_str(), (long long)positions[i]);
        for (int c = 0; c < k; ++c) std::fprintf(o.f, "\t%.6f", (double)loadings[i * (size_t)k + (size_t)c]);
        std::fputc('\n', o.f);
    }
}

// ---------------------------------------------------------------------------------------------- projection model (io.py's twin)
// P.eigensnp.model.tsv: "#gpca-model v1\tk=K\tfit_samples=N", "#eigenvalues\t%.17g ...", the header, then one row per PCA SNP with
// its f32 mean / s.d. / loadings in %.9g (reads back to the same f32)
struct ProjectionModel {
    std::vector<std::string> variant_ids, chromosomes, allele1, allele2;
    std::vector<int64_t> positions;
    std::vector<float> mean, sd, loadings;   // loadings [S][k]
    std::vector<double> eigenvalues;
    int k = 0;
    int64_t n_samples = 0;
};

inline void write_model(const std::string& prefix, const ProjectionModel& m) {
    OutFile o(prefix + ".eigensnp.model.tsv");
    std::fprintf(o.f, "#gpca-model v1\tk=%d\tfit_samples=%lld\n", m.k, (long long)m.n_samples);
    std::fputs("#eigenvalues", o.f);
    for (double v : m.eigenvalues) std::fprintf(o.f, "\t%.17g", v);
    std::fputs("\nVariantID\tChrom\tPos\tA1\tA2\tMean\tSD", o.f);
    for (int c = 1; c <= m.k; ++c) std::fprintf(o.f, "\tPC%d_loading", c);
    std::fputc('\n', o.f);
    for (size_t i = 0; i < m.variant_ids.size(); ++i) {
        std::fprintf(o.f, "%s\t%s\t%lld\t%s\t%s\t%.9g\t%.9g", m.variant_ids[i].c_str(), m.chromosomes[i].c_str(), (long long)m.positions[i],
                     m.allele1[i].c_str(), m.allele2[i].c_str(), (double)m.mean[i], (double)m.sd[i]);
        for (int c = 0; c < m.k; ++c) std::fprintf(o.f, "\t%.9g", (double)m.loadings[i * (size_t)m.k + (size_t)c]);
        std::fputc('\n', o.f);
    }
}

inline std::vector<std::string> split_tabs(const std::string& line) {
    std::vector<std::string> out;
    size_t a = 0;
    for (;;) {
        const size_t b = line.find('\t', a);
        out.push_back(line.substr(a, b == std::string::npos ? std::string::npos : b - a));
        if (b == std::string::npos) return out;
        a = b + 1;
    }
}

inline ProjectionModel read_model(const std::string& path) {
    std::ifstream f(path);
    if (!f) throw std::runtime_error("cannot open " + path);
    ProjectionModel m;
    std::string line;
    auto bad = [&](const std::string& why) { return std::runtime_error(path + ": " + why); };
    if (!std::getline(f, line)) throw bad("empty file");
    auto head = split_tabs(line);
    if (head.empty() || head[0] != "#gpca-model v1") throw bad("not a projection model (first line must start with '#gpca-model v1')");
    bool have_k = false, have_n = false;
    for (size_t i = 1; i < head.size(); ++i) {
        const size_t eq = head[i].find('=');
        if (eq == std::string::npos) continue;
        const std::string key = head[i].substr(0, eq), v = head[i].substr(eq + 1);
        try {
            if (key == "k") { m.k = std::stoi(v); have_k = true; }
            else if (key == "fit_samples") { m.n_samples = std::stoll(v); have_n = true; }
        } catch (...) { throw bad("the first line must carry k=<int> and fit_samples=<int>"); }
    }
    if (!have_k || !have_n || m.k < 1) throw bad("the first line must carry k=<int> and fit_samples=<int>");
    if (!std::getline(f, line)) throw bad("second line must be '#eigenvalues ...'");
    auto ev = split_tabs(line);
    if (ev.empty() || ev[0] != "#eigenvalues") throw bad("second line must be '#eigenvalues ...'");
    for (size_t i = 1; i < ev.size(); ++i) m.eigenvalues.push_back(std::stod(ev[i]));
    if (!std::getline(f, line)) throw bad("no header line");
    auto cols = split_tabs(line);
    const std::vector<std::string> want = {"VariantID", "Chrom", "Pos", "A1", "A2", "Mean", "SD"};
    if (cols.size() != 7 + (size_t)m.k || !std::equal(want.begin(), want.end(), cols.begin()))
        throw bad("bad header line (VariantID Chrom Pos A1 A2 Mean SD and " + std::to_string(m.k) + " loading columns expected)");
    int64_t ln = 3;
    while (std::getline(f, line)) {
        ++ln;
        if (line.empty()) continue;
        auto p = split_tabs(line);
        if (p.size() != 7 + (size_t)m.k)
            throw bad(std::to_string(ln) + ": " + std::to_string(p.size()) + " columns, " + std::to_string(7 + m.k) + " expected");
        m.variant_ids.push_back(p[0]); m.chromosomes.push_back(p[1]); m.positions.push_back(std::stoll(p[2]));
        m.allele1.push_back(p[3]); m.allele2.push_back(p[4]);
        m.mean.push_back((float)std::stod(p[5])); m.sd.push_back((float)std::stod(p[6]));
        for (int c = 0; c < m.k; ++c) m.loadings.push_back((float)std::stod(p[7 + c]));
    }
    return m;
}

// The model's rows per target row, matched by variant ID ('.' never matches; the first target row of a duplicated ID is the one used).
// Same (A1, A2): as is; swapped: mean -> 2 - mean, loadings -> -loadings; any other pair: dropped.
struct Alignment {
    std::vector<float> mean, sd, loadings;   // [M_target], [M_target], [M_target][k]; zero loading rows = outside the model
    int64_t matched = 0, flipped = 0, allele_mismatch = 0, absent = 0;
};
inline Alignment align_model(const ProjectionModel& m, const std::vector<std::string>& ids, const std::vector<std::string>& a1,
                             const std::vector<std::string>& a2) {
    const size_t M = ids.size(), k = (size_t)m.k;
    std::map<std::string, size_t> first;
    for (size_t i = 0; i < M; ++i) if (ids[i] != ".") first.emplace(ids[i], i);
    Alignment al;
    al.mean.assign(M, 0.f); al.sd.assign(M, 1.f); al.loadings.assign(M * k, 0.f);
    std::vector<char> seen(M, 0);
    for (size_t s = 0; s < m.variant_ids.size(); ++s) {
        const auto it = m.variant_ids[s] == "." ? first.end() : first.find(m.variant_ids[s]);
        if (it == first.end() || seen[it->second]) { al.absent++; continue; }
        const size_t i = it->second;
        const float* w = &m.loadings[s * k];
        if (a1[i] == m.allele1[s] && a2[i] == m.allele2[s]) {
            al.mean[i] = m.mean[s]; al.sd[i] = m.sd[s];
            for (size_t c = 0; c < k; ++c) al.loadings[i * k + c] = w[c];
        } else if (a1[i] == m.allele2[s] && a2[i] == m.allele1[s]) {
            al.mean[i] = 2.0f - m.mean[s]; al.sd[i] = m.sd[s];
            for (size_t c = 0; c < k; ++c) al.loadings[i * k + c] = -w[c];
            al.flipped++;
        } else { al.allele_mismatch++; continue; }
        seen[i] = 1;
        al.matched++;
    }
    return al;
}

// Q.projected.pca.tsv: SampleID, PC1..PCk ("{:.6}" as the other PC files), SNPsUsed
inline void write_projected(const std::string& prefix, const std::vector<std::string>& sample_names, const double* scores, int k,
                            const std::vector<int32_t>& used) {
    OutFile o(prefix + ".projected.pca.tsv");
    std::fputs("SampleID", o.f);
    for (int c = 1; c <= k; ++c) std::fprintf(o.f, "\tPC%d", c);
    std::fputs("\tSNPsUsed\n", o.f);
    for (size_t i = 0; i < sample_names.size(); ++i) {
        std::fputs(sample_names[i].c_str(), o.f);
        for (int c = 0; c < k; ++c) std::fprintf(o.f, "\t%.6f", scores[i * (size_t)k + (size_t)c]);
        std::fprintf(o.f, "\t%d\n", (int)used[i]);
    }
}

// GCTA's binary GRM layout, written band by band: P.grm.bin (f32 little-endian, lower triangle with the diagonal, packed row-major),
// P.grm.N.bin (f32, the number of SNPs behind each entry), P.grm.id (FID<TAB>IID per sample).  Bands come in row order, packed the same
// way (gpca_grm's output); close() checks that they covered the n (n + 1) / 2 entries and writes the ids.
class GrmWriter {
public:
    GrmWriter(const std::string& prefix, const std::vector<std::string>& family_ids, const std::vector<std::string>& sample_ids)
        : prefix_(prefix), fids_(family_ids), iids_(sample_ids), g_(prefix + ".grm.bin"), n_(prefix + ".grm.N.bin") {
        if (fids_.size() != iids_.size()) throw std::runtime_error("write_grm: one family ID per sample");
    }
    void add_band(const double* grm, const float* npairs, size_t entries) {
        std::vector<float> v(entries);
        for (size_t i = 0; i < entries; ++i) v[i] = (float)grm[i];
        if (std::fwrite(v.data(), 4, entries, g_.f) != entries || std::fwrite(npairs, 4, entries, n_.f) != entries)
            throw std::runtime_error("cannot write " + prefix_ + ".grm.bin / .grm.N.bin");
        total_ += entries;
    }
    void close() {
        const size_t n = iids_.size();
        if (total_ != n * (n + 1) / 2)
            throw std::runtime_error("write_grm: the bands hold " + std::to_string(total_) + " entries, " + std::to_string(n) + " samples need " +
                                     std::to_string(n * (n + 1) / 2));
        OutFile o(prefix_ + ".grm.id");
        for (size_t i = 0; i < n; ++i) std::fprintf(o.f, "%s\t%s\n", fids_[i].c_str(), iids_[i].c_str());
    }

private:
    std::string prefix_;
    std::vector<std::string> fids_, iids_;
    OutFile g_, n_;
    size_t total_ = 0;
};

// P.kin0 (KING-robust kinship), written band by band: `#FID1 IID1 FID2 IID2 NSNP HETHET IBS0 KINSHIP`, tab-separated, one line per
// pair of gpca_king's band order (ID1 the earlier sample in .fam order), the kinship as %.6f or nan; min_kinship (if set): only pairs
// with kinship >= it (io.write_kin0).
class Kin0Writer {
public:
    Kin0Writer(const std::string& prefix, const std::vector<std::string>& family_ids, const std::vector<std::string>& sample_ids,
               bool filter, double min_kinship)
        : prefix_(prefix), fids_(family_ids), iids_(sample_ids), f_(prefix + ".kin0"), filter_(filter), min_(min_kinship) {
        if (fids_.size() != iids_.size()) throw std::runtime_error("write_kin0: one family ID per sample");
        std::fputs("#FID1\tIID1\tFID2\tIID2\tNSNP\tHETHET\tIBS0\tKINSHIP\n", f_.f);
    }
    void add_band(int64_t row0, int64_t row1, const double* kin, const int32_t* counts) {
        if (row0 != next_) throw std::runtime_error("write_kin0: band [" + std::to_string(row0) + ", " + std::to_string(row1) + ") does not follow row " + std::to_string(next_));
        next_ = row1;
        size_t i = 0;
        for (int64_t j = row0; j < row1; ++j)
            for (int64_t k = 0; k < j; ++k, ++i) {
                const double v = kin[i];
                if (filter_ && !(v >= min_)) continue;
                char num[64];
                if (v != v) std::snprintf(num, sizeof num, "nan"); else std::snprintf(num, sizeof num, "%.6f", v);
                std::fprintf(f_.f, "%s\t%s\t%s\t%s\t%d\t%d\t%d\t%s\n", fids_[(size_t)k].c_str(), iids_[(size_t)k].c_str(), fids_[(size_t)j].c_str(),
                             iids_[(size_t)j].c_str(), counts[3 * i], counts[3 * i + 1], counts[3 * i + 2], num);
            }
    }
    void close() {
        if (!iids_.empty() && next_ != (int64_t)iids_.size())
            throw std::runtime_error("write_kin0: the bands end at row " + std::to_string(next_) + ", " + std::to_string(iids_.size()) + " samples need " + std::to_string(iids_.size()));
    }

private:
    std::string prefix_;
    std::vector<std::string> fids_, iids_;
    OutFile f_;
    bool filter_;
    double min_;
    int64_t next_ = 0;
};

// The greedy pruning rule of --gpca-king-cutoff (io.king_unrelated): while a related pair remains, the sample with the most remaining
// partners leaves, ties going to the later sample.  pairs: (i, j) sample indices.  Returns keep[n] (1 = in the fit).
inline std::vector<uint8_t> king_unrelated(int64_t n, const std::vector<std::pair<int64_t, int64_t>>& pairs) {
    std::vector<std::set<int64_t>> adj((size_t)n);
    for (const auto& p : pairs) {
        if (p.first == p.second || p.first < 0 || p.second < 0 || p.first >= n || p.second >= n) throw std::runtime_error("king_unrelated: bad pair");
        adj[(size_t)p.first].insert(p.second); adj[(size_t)p.second].insert(p.first);
    }
    std::vector<uint8_t> keep((size_t)n, 1);
    for (;;) {
        int64_t s = -1; size_t top = 0;
        for (int64_t i = 0; i < n; ++i)
            if (adj[(size_t)i].size() >= top && adj[(size_t)i].size() > 0) { top = adj[(size_t)i].size(); s = i; }
        if (s < 0) break;
        keep[(size_t)s] = 0;
        for (int64_t t : adj[(size_t)s]) adj[(size_t)t].erase(s);
        adj[(size_t)s].clear();
    }
    return keep;
}

// P.king.cutoff.in.id / P.king.cutoff.out.id: `#FID<TAB>IID`, then the samples of each set in .fam order
inline void write_king_cutoff_ids(const std::string& prefix, const std::vector<std::string>& family_ids, const std::vector<std::string>& sample_ids,
                                  const std::vector<uint8_t>& keep) {
    for (int want = 1; want >= 0; --want) {
        OutFile o(prefix + (want ? ".king.cutoff.in.id" : ".king.cutoff.out.id"));
        std::fputs("#FID\tIID\n", o.f);
        for (size_t i = 0; i < sample_ids.size(); ++i)
            if ((keep[i] != 0) == (want == 1)) std::fprintf(o.f, "%s\t%s\n", family_ids[i].c_str(), sample_ids[i].c_str());
    }
}

// P.pcrelate.kin and P.pcrelate.inbreed (PC-Relate), written band by band from gpca_pcrelate's output (the lower triangle WITH its
// diagonal): `#FID1 IID1 FID2 IID2 NSNP KINSHIP` per strictly lower pair (ID1 the earlier sample in .fam order), the kinship as %.6f or
// nan, only pairs with kinship >= min_kinship if that is set; `#FID IID NSNP F` per sample, F = 2 self-kinship - 1, never filtered
// (io.write_pcrelate).
class PcrelateWriter {
public:
    PcrelateWriter(const std::string& prefix, const std::vector<std::string>& family_ids, const std::vector<std::string>& sample_ids,
                   bool filter, double min_kinship)
        : fids_(family_ids), iids_(sample_ids), k_(prefix + ".pcrelate.kin"), i_(prefix + ".pcrelate.inbreed"), filter_(filter), min_(min_kinship) {
        if (fids_.size() != iids_.size()) throw std::runtime_error("write_pcrelate: one family ID per sample");
        std::fputs("#FID1\tIID1\tFID2\tIID2\tNSNP\tKINSHIP\n", k_.f);
        std::fputs("#FID\tIID\tNSNP\tF\n", i_.f);
    }
    void add_band(int64_t row0, int64_t row1, const double* kin, const int32_t* nsnp) {
        if (row0 != next_) throw std::runtime_error("write_pcrelate: band [" + std::to_string(row0) + ", " + std::to_string(row1) + ") does not follow row " + std::to_string(next_));
        next_ = row1;
        size_t i = 0;
        char num[64];
        for (int64_t a = row0; a < row1; ++a) {
            for (int64_t b = 0; b < a; ++b, ++i) {
                const double v = kin[i];
                if (filter_ && !(v >= min_)) continue;
                fmt(num, sizeof num, v);
                std::fprintf(k_.f, "%s\t%s\t%s\t%s\t%d\t%s\n", fids_[(size_t)b].c_str(), iids_[(size_t)b].c_str(), fids_[(size_t)a].c_str(),
                             iids_[(size_t)a].c_str(), nsnp[i], num);
            }
            fmt(num, sizeof num, 2.0 * kin[i] - 1.0);
            std::fprintf(i_.f, "%s\t%s\t%d\t%s\n", fids_[(size_t)a].c_str(), iids_[(size_t)a].c_str(), nsnp[i], num);
            ++i;
        }
    }
    void close() {
        if (!iids_.empty() && next_ != (int64_t)iids_.size())
            throw std::runtime_error("write_pcrelate: the bands end at row " + std::to_string(next_) + ", " + std::to_string(iids_.size()) + " samples need " + std::to_string(iids_.size()));
    }

private:
    static void fmt(char* buf, size_t n, double v) { if (v != v) std::snprintf(buf, n, "nan"); else std::snprintf(buf, n, "%.6f", v); }
    std::vector<std::string> fids_, iids_;
    OutFile k_, i_;
    bool filter_;
    double min_;
    int64_t next_ = 0;
};

// ---- windowed LD and LD pruning: the twins of io.parse_ld_window, io.ld_windows, io.ld_bands, io.ld_prune, io.maf_from_qc_detail and
// io.write_prune_ids (same rules, same error texts, byte-identical files) --------------------------------------------------------
struct LdWindow { bool bp; int64_t w; };   // bp: a span in base pairs; otherwise a count of variants (the SNP itself included)
inline LdWindow parse_ld_window(const std::string& text) {
    auto strip = [](std::string t) {
        size_t a = 0, b = t.size();
        while (a < b && std::isspace((unsigned char)t[a])) ++a;
        while (b > a && std::isspace((unsigned char)t[b - 1])) --b;
        return t.substr(a, b - a);
    };
    std::string t = strip(text);
    std::transform(t.begin(), t.end(), t.begin(), [](unsigned char c) { return (char)std::tolower(c); });
    const bool kb = t.size() >= 2 && t.compare(t.size() - 2, 2, "kb") == 0;
    const std::string num = kb ? strip(t.substr(0, t.size() - 2)) : t;
    const std::string bad = "bad LD window '" + text + "': ";
    char* end = nullptr;
    if (num.empty() || std::isspace((unsigned char)num[0])) throw std::runtime_error(bad + "expected a variant count such as 50 or a span such as 250kb");
    if (kb) {
        const double v = std::strtod(num.c_str(), &end);
        if (*end) throw std::runtime_error(bad + "expected a variant count such as 50 or a span such as 250kb");
        if (!(v > 0.0) || !std::isfinite(v)) throw std::runtime_error(bad + "the span must be positive");
        return LdWindow{true, (int64_t)std::nearbyint(v * 1000.0)};
    }
    const long long v = std::strtoll(num.c_str(), &end, 10);
    if (*end) throw std::runtime_error(bad + "expected a variant count such as 50 or a span such as 250kb");
    if (v < 2) throw std::runtime_error(bad + "a window in variants holds at least 2");
    return LdWindow{false, (int64_t)v};
}

// win_end [K] over the kept SNPs, in their order: SNP i is paired with the later SNPs j < win_end[i] of its chromosome run
inline std::vector<int64_t> ld_windows(const std::vector<std::string>& chromosomes, const std::vector<int64_t>& positions, const std::string& window) {
    const LdWindow lw = parse_ld_window(window);
    const int64_t K = (int64_t)chromosomes.size();
    if ((int64_t)positions.size() != K) throw std::runtime_error("ld_windows: one position per chromosome entry");
    std::vector<int64_t> win_end((size_t)K);
    std::set<std::string> seen;
    for (int64_t s = 0; s < K;) {
        const std::string c = normalize_chromosome_name(chromosomes[(size_t)s]);
        if (!seen.insert(c).second)
            throw std::runtime_error("ld_windows: chromosome '" + chromosomes[(size_t)s] + "' reappears at variant " + std::to_string(s) +
                                     " after another chromosome: sort the variants");
        int64_t e = s + 1;
        while (e < K && normalize_chromosome_name(chromosomes[(size_t)e]) == c) {
            if (positions[(size_t)e] < positions[(size_t)e - 1])
                throw std::runtime_error("ld_windows: the position of variant " + std::to_string(e) + " (" + std::to_string(positions[(size_t)e]) +
                                         ") is below that of the variant before it on chromosome '" + chromosomes[(size_t)e] + "': sort the variants");
            ++e;
        }
        int64_t hi = s;                                  // first SNP of the run beyond the window of i (positions are sorted: it only moves on)
        for (int64_t i = s; i < e; ++i) {
            if (!lw.bp) { win_end[(size_t)i] = std::min(i + lw.w, e); continue; }
            if (hi < i + 1) hi = i + 1;
            while (hi < e && positions[(size_t)hi] <= positions[(size_t)i] + lw.w) ++hi;
            win_end[(size_t)i] = hi;
        }
        s = e;
    }
    return win_end;
}

// the next row band [r0, r1) with (r1 - r0) * wmax <= max_slots (at least one row), wmax = its widest window (at least 1)
inline void ld_next_band(const std::vector<int64_t>& win_end, int64_t r0, int64_t max_slots, int64_t& r1, int64_t& wmax) {
    const int64_t K = (int64_t)win_end.size();
    auto width = [&](int64_t i) { return win_end[(size_t)i] - i - 1; };
    r1 = r0 + 1; wmax = std::max<int64_t>(width(r0), 1);
    while (r1 < K) {
        const int64_t w2 = std::max(wmax, width(r1));
        if ((r1 + 1 - r0) * w2 > max_slots) break;
        wmax = w2; ++r1;
    }
}

// one band of the pruning rule (io.ld_prune): above [r1 - r0][words] as gpca_ld_window writes it; bands come in row order
inline void ld_prune_band(const std::vector<int64_t>& win_end, int64_t r0, int64_t r1, const std::vector<uint64_t>& above, int64_t words,
                          const std::vector<double>& maf, std::vector<uint8_t>& inset) {
    for (int64_t i = r0; i < r1; ++i) {
        if (!inset[(size_t)i]) continue;
        const uint64_t* row = above.data() + (size_t)(i - r0) * (size_t)words;
        const int64_t n = win_end[(size_t)i] - i - 1;
        for (int64_t d = 0; d < n; ++d) {
            if (!((row[d >> 6] >> (d & 63)) & 1u)) continue;
            const int64_t j = i + 1 + d;
            if (!inset[(size_t)j]) continue;
            if (maf[(size_t)j] > maf[(size_t)i]) { inset[(size_t)i] = 0; break; }
            inset[(size_t)j] = 0;
        }
    }
}

inline double maf_from_counts(uint32_t n_valid, uint32_t n_het, uint32_t n_hom2) {
    if (n_valid == 0) return 0.0;
    const double p = ((double)n_het + 2.0 * (double)n_hom2) / (2.0 * (double)n_valid);
    return std::min(p, 1.0 - p);
}

// P.prune.in / P.prune.out: one variant ID per line, in the order given
inline void write_prune_ids(const std::string& prefix, const std::vector<std::string>& variant_ids, const std::vector<uint8_t>& inset) {
    if (variant_ids.size() != inset.size()) throw std::runtime_error("write_prune_ids: one in-set flag per variant ID");
    for (int want = 1; want >= 0; --want) {
        OutFile o(prefix + (want ? ".prune.in" : ".prune.out"));
        for (size_t i = 0; i < variant_ids.size(); ++i)
            if ((inset[i] != 0) == (want == 1)) std::fprintf(o.f, "%s\n", variant_ids[i].c_str());
    }
}

// ---- LD scores and LD-score regression: the twins of io.ld_score_sum, io.write_ldscore and io.write_ldsc_summary (same rules,
// byte-identical files) -----------------------------------------------------------------------------------------------------------
// adds one band of gpca_ld_score (its span from row0: score and, when not null, partners) into the K-long sums
inline void ld_score_add_band(std::vector<int64_t>& acc, std::vector<int64_t>& part, int64_t row0, const std::vector<int64_t>& score,
                              const std::vector<int32_t>* partners) {
    if (row0 < 0 || (size_t)row0 + score.size() > acc.size() || part.size() != acc.size())
        throw std::runtime_error("ld_score_sum: the band at row " + std::to_string(row0) + " holds " + std::to_string(score.size()) + " sums, " +
                                 std::to_string(acc.size()) + " rows are there");
    if (partners && partners->size() != score.size()) throw std::runtime_error("ld_score_sum: partners and score of a band have one length");
    for (size_t t = 0; t < score.size(); ++t) {
        acc[(size_t)row0 + t] += score[t];
        if (partners) part[(size_t)row0 + t] += (*partners)[t];
    }
}

inline std::string g6_or_na(double v) {
    char b[48];
    if (v != v) return "NA";
    std::snprintf(b, sizeof b, "%.6g", v);
    return b;
}

// P.l2.ldscore (tab-separated, header `CHR SNP BP L2`, L2 as %.6g: ldsc's column layout), P.l2.M (the number of SNPs summed over) and
// P.l2.M_5_50 (those with MAF > 0.05)
inline void write_ldscore(const std::string& prefix, const std::vector<std::string>& chromosomes, const std::vector<std::string>& ids,
                          const std::vector<int64_t>& positions, const std::vector<double>& l2, const std::vector<double>& maf) {
    const size_t n = ids.size();
    if (chromosomes.size() != n || positions.size() != n || l2.size() != n || maf.size() != n)
        throw std::runtime_error("write_ldscore: one entry per SNP in every column");
    ensure_parent(prefix);
    {
        OutFile o(prefix + ".l2.ldscore");
        std::fputs("CHR\tSNP\tBP\tL2\n", o.f);
        for (size_t i = 0; i < n; ++i)
            std::fprintf(o.f, "%s\t%s\t%lld\t%s\n", chromosomes[i].c_str(), ids[i].c_str(), (long long)positions[i], g6_or_na(l2[i]).c_str());
    }
    long long common = 0;
    for (double m : maf) common += m > 0.05;
    { OutFile o(prefix + ".l2.M"); std::fprintf(o.f, "%zu\n", n); }
    { OutFile o(prefix + ".l2.M_5_50"); std::fprintf(o.f, "%lld\n", common); }
}

// P.ldsc.summary: one tab-separated line per trait; fit = the ten values of gpca_ldsc_fit, or empty where the regression was refused
// (its numbers are NA then).  N and M_USED are integers, the others %.6g, NaN as NA.
struct LdscRow { std::string trait, test; int64_t n; std::vector<double> fit; };
inline void write_ldsc_summary(const std::string& prefix, const std::vector<LdscRow>& rows) {
    ensure_parent(prefix);
    OutFile o(prefix + ".ldsc.summary");
    std::fputs("#TRAIT\tTEST\tN\tM_USED\tMEAN_CHI2\tLAMBDA_GC\tINTERCEPT\tINTERCEPT_SE\tH2\tH2_SE\tRATIO\tRATIO_SE\n", o.f);
    for (const LdscRow& r : rows) {
        if (r.test != "LINEAR" && r.test != "LOGISTIC") throw std::runtime_error("write_ldsc_summary: TEST is LINEAR or LOGISTIC, not '" + r.test + "'");
        std::fprintf(o.f, "%s\t%s\t%lld", r.trait.c_str(), r.test.c_str(), (long long)r.n);
        if (r.fit.size() != 10) { for (int k = 0; k < 9; ++k) std::fputs("\tNA", o.f); }
        else {
            std::fprintf(o.f, "\t%lld", (long long)r.fit[0]);
            for (int k = 1; k <= 8; ++k) std::fprintf(o.f, "\t%s", g6_or_na(r.fit[(size_t)k]).c_str());
        }
        std::fputs("\n", o.f);
    }
}

// ---- linear association scan: the twins of io.read_pheno, io.align_pheno, io.assoc_bands and io.write_assoc (same rules, same error
// texts, byte-identical files) --------------------------------------------------------------------------------------------------------
struct PhenoTable {
    std::vector<std::string> family_ids, sample_ids, names;
    std::vector<double> values;      // [samples][names], NaN = missing
};

// A whitespace-separated phenotype or covariate table.  The header `FID IID name...` (a leading '#' allowed) is required; `NA` and `nan`
// in any letter case mean missing; a repeated (FID, IID) is refused.
inline PhenoTable read_pheno(const std::string& path) {
    std::ifstream in(path);
    if (!in) throw std::runtime_error("cannot open " + path);
    PhenoTable t;
    bool have_header = false;
    std::set<std::pair<std::string, std::string>> seen;
    std::string line;
    const std::string need = path + ": the header `FID IID name...` with at least one column is required";
    auto upper = [](std::string s) { for (char& c : s) c = (char)std::toupper((unsigned char)c); return s; };
    for (int64_t ln = 1; std::getline(in, line); ++ln) {
        const std::vector<std::string> p = split_ws(line);
        if (p.empty()) continue;
        if (!have_header) {
            if (p.size() < 3 || upper(p[0].substr(std::min(p[0].find_first_not_of('#'), p[0].size()))) != "FID" || upper(p[1]) != "IID")
                throw std::runtime_error(need);
            t.names.assign(p.begin() + 2, p.end());
            if (std::set<std::string>(t.names.begin(), t.names.end()).size() != t.names.size())
                throw std::runtime_error(path + ": a column name is repeated");
            have_header = true;
            continue;
        }
        const std::string at = path + ":" + std::to_string(ln) + ": ";
        if (p.size() != 2 + t.names.size())
            throw std::runtime_error(at + std::to_string(p.size()) + " fields, the header has " + std::to_string(2 + t.names.size()));
        if (!seen.insert({p[0], p[1]}).second) throw std::runtime_error(at + "sample " + p[0] + " " + p[1] + " appears twice");
        for (size_t c = 2; c < p.size(); ++c) {
            const std::string lo = upper(p[c]);
            if (lo == "NA" || lo == "NAN") { t.values.push_back(std::nan("")); continue; }
            char* end = nullptr;
            const double v = std::strtod(p[c].c_str(), &end);
            if (end == p[c].c_str() || *end || p[c].find_first_of("xX_") != std::string::npos) throw std::runtime_error(at + "`" + p[c] + "` is not a number");
            t.values.push_back(v);
        }
        t.family_ids.push_back(p[0]); t.sample_ids.push_back(p[1]);
    }
    if (!have_header) throw std::runtime_error(need);
    return t;
}

// The table's rows in .fam order, matched by (FID, IID): [samples][columns]; a sample absent from the table is missing (NaN) in every
// column; rows of the table that name no sample of the .fam are ignored.
inline std::vector<double> align_pheno(const PhenoTable& t, const std::vector<std::string>& family_ids, const std::vector<std::string>& sample_ids) {
    std::map<std::pair<std::string, std::string>, size_t> at;
    for (size_t r = 0; r < t.sample_ids.size(); ++r) at[{t.family_ids[r], t.sample_ids[r]}] = r;
    const size_t c = t.names.size();
    std::vector<double> out(sample_ids.size() * c, std::nan(""));
    for (size_t n = 0; n < sample_ids.size(); ++n) {
        const auto it = at.find({family_ids[n], sample_ids[n]});
        if (it != at.end()) std::copy(t.values.begin() + it->second * c, t.values.begin() + (it->second + 1) * c, out.begin() + n * c);
    }
    return out;
}

// [row0, row1) bands of the K kept rows whose xb workspace (rows x L doubles) holds at most max_values entries (at least one row)
inline std::vector<std::pair<int64_t, int64_t>> assoc_bands(int64_t K, int64_t L, int64_t max_values = (int64_t)1 << 26) {
    const int64_t step = std::max<int64_t>(max_values / std::max<int64_t>(L, 1), 1);
    std::vector<std::pair<int64_t, int64_t>> out;
    for (int64_t r0 = 0; r0 < K; r0 += step) out.emplace_back(r0, std::min(r0 + step, K));
    return out;
}

// P.<trait>.assoc.linear: one tab-separated line per SNP, `#CHROM POS ID A1 OBS_CT A1_FREQ BETA SE T_STAT LOG10P`; numbers as %.6g, NaN
// as NA, OBS_CT as an integer; rows are added band by band
class AssocWriter {
public:
    AssocWriter(const std::string& prefix, const std::string& trait) : o_(prefix + "." + trait + ".assoc.linear") {
        std::fputs("#CHROM\tPOS\tID\tA1\tOBS_CT\tA1_FREQ\tBETA\tSE\tT_STAT\tLOG10P\n", o_.f);
    }
    void add_row(const std::string& chrom, int64_t pos, const std::string& id, const std::string& a1, double n_obs, double a1_freq, double beta,
                 double se, double t, double log10p) {
        char b[5][48];
        const double v[5] = {a1_freq, beta, se, t, log10p};
        for (int i = 0; i < 5; ++i) { if (v[i] != v[i]) std::snprintf(b[i], sizeof b[i], "NA"); else std::snprintf(b[i], sizeof b[i], "%.6g", v[i]); }
        std::fprintf(o_.f, "%s\t%lld\t%s\t%s\t%lld\t%s\t%s\t%s\t%s\t%s\n", chrom.c_str(), (long long)pos, id.c_str(), a1.c_str(), (long long)n_obs, b[0], b[1],
                     b[2], b[3], b[4]);
    }

private:
    OutFile o_;
};

// ---- many-trait QTL scan: the twins of io.assoc_qtl_bands, io.qtl_best_merge, io.write_qtl_hits and io.write_qtl_best ---------------
constexpr int64_t kQtlHitsPerPairs = 4096;                   // the record buffer holds one pair in this many of a band
constexpr int64_t kQtlBandWorkMax = (int64_t)1 << 47;        // rows x N x T of one call
// [row0, row1) bands of the K kept rows for gpca_assoc_qtl with a record buffer of cap hits: whole blocks of 128 rows (at least one)
// such that cap holds one pair in kQtlHitsPerPairs of the band's rows x T pairs and rows x N x T stays within kQtlBandWorkMax
inline std::vector<std::pair<int64_t, int64_t>> assoc_qtl_bands(int64_t K, int64_t T, int64_t N, int64_t cap) {
    T = std::max<int64_t>(T, 1); N = std::max<int64_t>(N, 1); cap = std::max<int64_t>(cap, 1);
    int64_t step = std::min(cap * kQtlHitsPerPairs / T, kQtlBandWorkMax / (N * T));
    step = std::max<int64_t>(step / 128 * 128, 128);
    std::vector<std::pair<int64_t, int64_t>> out;
    for (int64_t r0 = 0; r0 < K; r0 += step) out.emplace_back(r0, std::min(r0 + step, K));
    return out;
}

// the running best over bands in ascending row order: a band's (r2, row) replaces a trait's entry when the trait has none yet (row < 0)
// or the band's r2 is strictly larger, so a tie stays with the lower row
inline void qtl_best_merge(std::vector<double>& best_r2, std::vector<int64_t>& best_row, const std::vector<double>& band_r2,
                           const std::vector<int64_t>& band_row) {
    for (size_t t = 0; t < best_r2.size(); ++t)
        if (band_row[t] >= 0 && (best_row[t] < 0 || band_r2[t] > best_r2[t])) { best_r2[t] = band_r2[t]; best_row[t] = band_row[t]; }
}

// P.qtl.hits: one tab-separated line per hit in the order given (the scan's: ascending (row, trait)), `#CHROM POS ID A1 TRAIT OBS_CT
// A1_FREQ BETA SE T_STAT LOG10P`; numbers as %.6g, NaN as NA, OBS_CT as an integer; hits are added band by band
class QtlHitsWriter {
public:
    explicit QtlHitsWriter(const std::string& prefix) : o_(prefix + ".qtl.hits") {
        std::fputs("#CHROM\tPOS\tID\tA1\tTRAIT\tOBS_CT\tA1_FREQ\tBETA\tSE\tT_STAT\tLOG10P\n", o_.f);
    }
    void add_hit(const std::string& chrom, int64_t pos, const std::string& id, const std::string& a1, const std::string& trait, double n_obs,
                 double a1_freq, double beta, double se, double t, double log10p) {
        char b[5][48];
        const double v[5] = {a1_freq, beta, se, t, log10p};
        for (int i = 0; i < 5; ++i) { if (v[i] != v[i]) std::snprintf(b[i], sizeof b[i], "NA"); else std::snprintf(b[i], sizeof b[i], "%.6g", v[i]); }
        std::fprintf(o_.f, "%s\t%lld\t%s\t%s\t%s\t%lld\t%s\t%s\t%s\t%s\t%s\n", chrom.c_str(), (long long)pos, id.c_str(), a1.c_str(), trait.c_str(),
                     (long long)n_obs, b[0], b[1], b[2], b[3], b[4]);
    }

private:
    OutFile o_;
};

// P.qtl.best: one tab-separated line per trait, `#TRAIT CHROM POS ID A1 BETA SE T_STAT LOG10P N_TESTS`: the SNP with the largest r2 for
// the trait over all bands and the number of live SNPs it was chosen from; add_none: a trait without a live SNP (NA in the SNP's columns)
class QtlBestWriter {
public:
    explicit QtlBestWriter(const std::string& prefix) : o_(prefix + ".qtl.best") {
        std::fputs("#TRAIT\tCHROM\tPOS\tID\tA1\tBETA\tSE\tT_STAT\tLOG10P\tN_TESTS\n", o_.f);
    }
    void add_trait(const std::string& trait, const std::string& chrom, int64_t pos, const std::string& id, const std::string& a1, double beta,
                   double se, double t, double log10p, int64_t n_tests) {
        char b[4][48];
        const double v[4] = {beta, se, t, log10p};
        for (int i = 0; i < 4; ++i) { if (v[i] != v[i]) std::snprintf(b[i], sizeof b[i], "NA"); else std::snprintf(b[i], sizeof b[i], "%.6g", v[i]); }
        std::fprintf(o_.f, "%s\t%s\t%lld\t%s\t%s\t%s\t%s\t%s\t%s\t%lld\n", trait.c_str(), chrom.c_str(), (long long)pos, id.c_str(), a1.c_str(), b[0], b[1],
                     b[2], b[3], (long long)n_tests);
    }
    void add_none(const std::string& trait, int64_t n_tests) {
        std::fprintf(o_.f, "%s\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\t%lld\n", trait.c_str(), (long long)n_tests);
    }

private:
    OutFile o_;
};

// ---- cis-QTL mapping: the twins of io.qtl_cis_windows, io.read_trait_pos, io.assoc_qtl_cis_bands and io.write_qtl_cis -----------------
constexpr int64_t kQtlCisResultBytesMax = (int64_t)256 << 20;      // perm_r2 [G][P] f64 of one call
// win [G][2] for gpca_assoc_qtl_cis: [lo, hi) over the kept SNPs given (in their order) with |pos - trait_pos| <= window_bp on the trait's
// chromosome; lo = hi where none qualifies, [0, 0) for a chromosome the SNPs do not have.  Ordered as ld_windows requires.
inline std::vector<int64_t> qtl_cis_windows(const std::vector<std::string>& chromosomes, const std::vector<int64_t>& positions,
                                            const std::vector<std::string>& trait_chrom, const std::vector<int64_t>& trait_pos, int64_t window_bp) {
    const int64_t K = (int64_t)chromosomes.size();
    if ((int64_t)positions.size() != K) throw std::runtime_error("qtl_cis_windows: one position per chromosome entry");
    if (trait_chrom.size() != trait_pos.size()) throw std::runtime_error("qtl_cis_windows: one position per trait chromosome");
    std::map<std::string, std::pair<int64_t, int64_t>> runs;
    for (int64_t s = 0; s < K;) {
        const std::string c = normalize_chromosome_name(chromosomes[(size_t)s]);
        if (runs.count(c))
            throw std::runtime_error("qtl_cis_windows: chromosome '" + chromosomes[(size_t)s] + "' reappears at variant " + std::to_string(s) +
                                     " after another chromosome: sort the variants");
        int64_t e = s + 1;
        while (e < K && normalize_chromosome_name(chromosomes[(size_t)e]) == c) {
            if (positions[(size_t)e] < positions[(size_t)e - 1])
                throw std::runtime_error("qtl_cis_windows: the position of variant " + std::to_string(e) + " (" + std::to_string(positions[(size_t)e]) +
                                         ") is below that of the variant before it on chromosome '" + chromosomes[(size_t)e] + "': sort the variants");
            ++e;
        }
        runs[c] = {s, e};
        s = e;
    }
    std::vector<int64_t> win(2 * trait_chrom.size(), 0);
    for (size_t g = 0; g < trait_chrom.size(); ++g) {
        const auto it = runs.find(normalize_chromosome_name(trait_chrom[g]));
        if (it == runs.end()) continue;
        const auto b = positions.begin() + it->second.first, e = positions.begin() + it->second.second;
        win[2 * g] = it->second.first + (std::lower_bound(b, e, trait_pos[g] - window_bp) - b);
        win[2 * g + 1] = it->second.first + (std::upper_bound(b, e, trait_pos[g] + window_bp) - b);
    }
    return win;
}

// A `TRAIT CHROM POS` table (that header; whitespace-separated): trait -> (chrom, pos); a later line of a trait replaces an earlier one
inline std::map<std::string, std::pair<std::string, int64_t>> read_trait_pos(const std::string& path) {
    std::ifstream in(path);
    if (!in) throw std::runtime_error("cannot open " + path);
    std::map<std::string, std::pair<std::string, int64_t>> out;
    std::string line;
    std::getline(in, line);
    const std::vector<std::string> head = split_ws(line);
    if (head != std::vector<std::string>{"TRAIT", "CHROM", "POS"}) throw std::runtime_error(path + ": the header must be 'TRAIT CHROM POS'");
    for (int64_t ln = 2; std::getline(in, line); ++ln) {
        const std::vector<std::string> t = split_ws(line);
        if (t.empty()) continue;
        if (t.size() != 3) throw std::runtime_error(path + ": line " + std::to_string(ln) + " does not hold TRAIT CHROM POS");
        const std::string& p = t[2];
        const size_t d0 = (p[0] == '+' || p[0] == '-') ? 1 : 0;
        bool ok = p.size() > d0 && p.size() <= 18;
        for (size_t i = d0; i < p.size(); ++i) ok = ok && p[i] >= '0' && p[i] <= '9';
        if (!ok) throw std::runtime_error(path + ": line " + std::to_string(ln) + ": the position '" + p + "' is not an integer");
        out[t[0]] = {t[1], std::stoll(p)};
    }
    return out;
}

// [g0, g1) bands of the G traits for gpca_assoc_qtl_cis such that perm_r2 [g1 - g0][P] (f64) stays within kQtlCisResultBytesMax (at
// least one trait per band; one band when P = 0)
inline std::vector<std::pair<int64_t, int64_t>> assoc_qtl_cis_bands(int64_t G, int64_t P) {
    const int64_t step = P > 0 ? std::max<int64_t>(kQtlCisResultBytesMax / (8 * P), 1) : std::max<int64_t>(G, 1);
    std::vector<std::pair<int64_t, int64_t>> out;
    for (int64_t g0 = 0; g0 < G; g0 += step) out.emplace_back(g0, std::min(g0 + step, G));
    return out;
}

// P.qtl.cis: one tab-separated line per trait in the order added, `#TRAIT CHROM POS N_VAR ID VAR_POS A1 BETA SE T_STAT LOG10P_NOMINAL
// TRUE_DF SHAPE1 SHAPE2 PVAL_PERM LOG10P_BETA`; numbers as %.6g, NaN as NA.  add_no_pos: a trait without a position (NA in every column
// after the name); add_empty: a trait whose window holds no live SNP (its position, N_VAR = 0, NA from ID on)
class QtlCisWriter {
public:
    explicit QtlCisWriter(const std::string& prefix) : o_(prefix + ".qtl.cis") {
        std::fputs("#TRAIT\tCHROM\tPOS\tN_VAR\tID\tVAR_POS\tA1\tBETA\tSE\tT_STAT\tLOG10P_NOMINAL\tTRUE_DF\tSHAPE1\tSHAPE2\tPVAL_PERM\tLOG10P_BETA\n", o_.f);
    }
    void add_no_pos(const std::string& trait) { std::fprintf(o_.f, "%s\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n", trait.c_str()); }
    void add_empty(const std::string& trait, const std::string& chrom, int64_t pos) {
        std::fprintf(o_.f, "%s\t%s\t%lld\t0\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n", trait.c_str(), chrom.c_str(), (long long)pos);
    }
    // v [9] = beta, se, t, log10p_nominal, true_df, shape1, shape2, pval_perm, log10p_beta
    void add_trait(const std::string& trait, const std::string& chrom, int64_t pos, int64_t n_var, const std::string& id, int64_t var_pos,
                   const std::string& a1, const double* v) {
        std::fprintf(o_.f, "%s\t%s\t%lld\t%lld\t%s\t%lld\t%s", trait.c_str(), chrom.c_str(), (long long)pos, (long long)n_var, id.c_str(), (long long)var_pos,
                     a1.c_str());
        for (int i = 0; i < 9; ++i) { if (v[i] != v[i]) std::fputs("\tNA", o_.f); else std::fprintf(o_.f, "\t%.6g", v[i]); }
        std::fputc('\n', o_.f);
    }

private:
    OutFile o_;
};

// ---- logistic score scan: the twins of io.binary_trait, io.assoc_score_groups, io.assoc_score_bands and io.write_assoc_logistic ------
// true when column c of the table is binary: its present (non-NaN) values are exactly {0, 1} (1 = case) or exactly {1, 2} (plink's
// coding, 2 = case); *shift = what to take off a value to reach the 0 / 1 coding.  A column with one class only is not binary.
inline bool binary_trait(const PhenoTable& t, size_t c, double* shift) {
    const size_t nc = t.names.size();
    bool has[3] = {false, false, false};
    for (size_t r = 0; r * nc + c < t.values.size(); ++r) {
        const double v = t.values[r * nc + c];
        if (v != v) continue;
        if (v == 0.0) has[0] = true; else if (v == 1.0) has[1] = true; else if (v == 2.0) has[2] = true; else return false;
    }
    if (has[0] && has[1] && !has[2]) { if (shift) *shift = 0.0; return true; }
    if (!has[0] && has[1] && has[2]) { if (shift) *shift = 1.0; return true; }
    return false;
}

constexpr int64_t kAssocScoreMaxColumns = 64;
// [t0, t1) groups of T case / control traits, floor(64 / (Pc + 3)) to a group
inline std::vector<std::pair<int64_t, int64_t>> assoc_score_groups(int64_t T, int64_t Pc) {
    const int64_t g = kAssocScoreMaxColumns / (Pc + 3);
    if (g < 1) throw std::runtime_error(std::to_string(Pc) + " covariates + 3 are more than " + std::to_string(kAssocScoreMaxColumns) + " columns");
    std::vector<std::pair<int64_t, int64_t>> out;
    for (int64_t t0 = 0; t0 < T; t0 += g) out.emplace_back(t0, std::min(t0 + g, T));
    return out;
}
inline std::vector<std::pair<int64_t, int64_t>> assoc_score_bands(int64_t K, int64_t T, int64_t Pc, int64_t max_values = (int64_t)1 << 26) {
    return assoc_bands(K, T * (Pc + 3), max_values);
}

// the rule of gpca_assoc_logistic_spa's cutoff (io.spa_z_ok): at least 0.5, or inf (no correction); NaN is refused
inline bool spa_z_ok(double x) { return x >= 0.5; }
// the rule of gpca_assoc_logistic_firth's cutoff (io.firth_z_ok): at least 0, or inf (no correction); NaN is refused
inline bool firth_z_ok(double x) { return x >= 0.0; }

// P.<trait>.assoc.logistic: one tab-separated line per SNP, `#CHROM POS ID A1 OBS_CT A1_FREQ BETA SE Z_STAT LOG10P`; numbers as %.6g,
// NaN as NA, OBS_CT as an integer; rows are added band by band.  spa = true adds the column `SPA`: N, Y, F for the status 0, 1, 2 of the
// saddle-point correction (gpca_assoc_logistic_spa), NA where LOG10P is NA.  firth = true (not both) adds the column `FIRTH` in the same
// way for the Firth correction (gpca_assoc_logistic_firth); the caller passes Firth's BETA and SE on the rows with status 1
class AssocLogisticWriter {
public:
    AssocLogisticWriter(const std::string& prefix, const std::string& trait, bool spa = false, bool firth = false)
        : o_(prefix + "." + trait + ".assoc.logistic"), spa_(spa || firth) {
        if (spa && firth) throw std::runtime_error("AssocLogisticWriter: spa or firth, not both");
        std::fputs("#CHROM\tPOS\tID\tA1\tOBS_CT\tA1_FREQ\tBETA\tSE\tZ_STAT\tLOG10P", o_.f);
        std::fputs(spa ? "\tSPA\n" : (firth ? "\tFIRTH\n" : "\n"), o_.f);
    }
    void add_row(const std::string& chrom, int64_t pos, const std::string& id, const std::string& a1, double n_obs, double a1_freq, double beta,
                 double se, double z, double log10p, int spa_status = 0) {
        char b[5][48];
        const double v[5] = {a1_freq, beta, se, z, log10p};
        for (int i = 0; i < 5; ++i) { if (v[i] != v[i]) std::snprintf(b[i], sizeof b[i], "NA"); else std::snprintf(b[i], sizeof b[i], "%.6g", v[i]); }
        const char* tail = !spa_ ? "" : (log10p != log10p ? "\tNA" : (spa_status == 1 ? "\tY" : (spa_status == 2 ? "\tF" : "\tN")));
        std::fprintf(o_.f, "%s\t%lld\t%s\t%s\t%lld\t%s\t%s\t%s\t%s\t%s%s\n", chrom.c_str(), (long long)pos, id.c_str(), a1.c_str(), (long long)n_obs, b[0], b[1],
                     b[2], b[3], b[4], tail);
    }

private:
    OutFile o_;
    bool spa_;
};

// ---- gene-level set tests of the logistic score scan: the twins of io.read_set_list, io.set_weights, io.set_maf_ok,
// io.assoc_set_groups and io.write_assoc_set ---------------------------------------------------------------------------------------
constexpr int64_t kAssocSetMaxRows = 128;
struct VariantSet {
    std::string name, chrom;
    int64_t pos = 0;
    std::vector<int64_t> rows;   // kept rows (PCA-SNP order) of the listed IDs that are among the QC-kept SNPs: ascending, each once
};
// regenie's set list: one set per line, `NAME CHROM POS ID1,ID2,...` separated by blanks or tabs (empty lines and lines that start with
// # are skipped).  kept_ids: the IDs of the QC-kept SNPs in PCA-SNP order; an ID that is not among them is dropped, an ID that occurs
// twice among them means its first row, and an ID listed twice in a set counts once.  Throws with the file and the line; the text
// "cannot open" alone when the file cannot be read.
inline std::vector<VariantSet> read_set_list(const std::string& path, const std::vector<std::string>& kept_ids) {
    std::unordered_map<std::string, int64_t> at;
    for (size_t i = 0; i < kept_ids.size(); ++i) at.emplace(kept_ids[i], (int64_t)i);
    std::ifstream f(path);
    if (!f) throw std::runtime_error("cannot open " + path);
    std::vector<VariantSet> out;
    std::string line;
    for (int64_t ln = 1; std::getline(f, line); ++ln) {
        const std::vector<std::string> p = split_ws(line);
        if (p.empty() || p[0][0] == '#') continue;
        const std::string where = path + ":" + std::to_string(ln) + ": ";
        if (p.size() != 4) throw std::runtime_error(where + "`NAME CHROM POS ID1,ID2,...` is required");
        VariantSet v;
        v.name = p[0]; v.chrom = p[1];
        {
            const std::string& t = p[2];
            size_t i = (t[0] == '-' || t[0] == '+') ? 1 : 0;
            bool ok = i < t.size() && t.size() - i <= 18;
            for (size_t k = i; k < t.size(); ++k) ok = ok && t[k] >= '0' && t[k] <= '9';
            if (!ok) throw std::runtime_error(where + "`" + t + "` is not a position");
            v.pos = std::stoll(t);
        }
        size_t b = 0;
        while (b <= p[3].size()) {
            size_t e = p[3].find(',', b);
            if (e == std::string::npos) e = p[3].size();
            const auto it = at.find(p[3].substr(b, e - b));
            if (it != at.end()) v.rows.push_back(it->second);
            b = e + 1;
        }
        std::sort(v.rows.begin(), v.rows.end());
        v.rows.erase(std::unique(v.rows.begin(), v.rows.end()), v.rows.end());
        out.push_back(std::move(v));
    }
    return out;
}
// the weight of a variant from its A1 frequency: beta = the Beta(maf; 1, 25) density 25 (1 - maf)^24 with maf = min(f, 1 - f) (the power
// by three squarings and one product, as io.set_weights takes it), otherwise (flat) 1
inline double set_weight(double a1_freq, bool beta) {
    if (!beta) return 1.0;
    const double q = 1.0 - std::min(a1_freq, 1.0 - a1_freq), q2 = q * q, q4 = q2 * q2, q8 = q4 * q4;
    return 25.0 * ((q8 * q8) * q8);
}
// a variant enters a set: min(f, 1 - f) <= max_maf (a variant without an observed call, f = NaN, does not)
inline bool set_maf_ok(double a1_freq, double max_maf) { return a1_freq == a1_freq && std::min(a1_freq, 1.0 - a1_freq) <= max_maf; }
// [s0, s1) groups of consecutive sets (sizes = their row counts, each 1 .. 128) for one gpca_assoc_logistic_set call each: the listed
// rows' workspace (rows x T (Pc + 3) doubles) and Phi (T m (m + 1) / 2 doubles per set) hold at most max_values entries each
inline std::vector<std::pair<int64_t, int64_t>> assoc_set_groups(const std::vector<int64_t>& sizes, int64_t T, int64_t Pc, int64_t max_values = (int64_t)1 << 26) {
    std::vector<std::pair<int64_t, int64_t>> out;
    int64_t s0 = 0, rows = 0, tri = 0;
    for (int64_t s = 0; s < (int64_t)sizes.size(); ++s) {
        const int64_t m = sizes[(size_t)s];
        int64_t r = rows + m, t = tri + m * (m + 1) / 2;
        if (s > s0 && (r * T * (Pc + 3) > max_values || t * T > max_values)) {
            out.emplace_back(s0, s);
            s0 = s; r = m; t = m * (m + 1) / 2;
        }
        rows = r; tri = t;
    }
    if ((int64_t)sizes.size() > s0) out.emplace_back(s0, (int64_t)sizes.size());
    return out;
}
// P.<trait>.assoc.set: one tab-separated line per set, `#SET CHROM POS N_VAR N_USED BURDEN_BETA BURDEN_SE BURDEN_Z BURDEN_LOG10P SKAT_Q
// SKAT_LOG10P SKAT`; numbers as %.6g, NaN as NA; SKAT = Y, N, F for the status 1, 0, 2 of gpca_set_test (NA where SKAT_LOG10P is NA).
// out = gpca_set_test's ten values, or NULL (no test was made: everything after N_VAR is NA)
class AssocSetWriter {
public:
    AssocSetWriter(const std::string& prefix, const std::string& trait) : o_(prefix + "." + trait + ".assoc.set") {
        std::fputs("#SET\tCHROM\tPOS\tN_VAR\tN_USED\tBURDEN_BETA\tBURDEN_SE\tBURDEN_Z\tBURDEN_LOG10P\tSKAT_Q\tSKAT_LOG10P\tSKAT\n", o_.f);
    }
    void add_row(const VariantSet& s, int64_t n_var, const double* out) {
        std::fprintf(o_.f, "%s\t%s\t%lld\t%lld", s.name.c_str(), s.chrom.c_str(), (long long)s.pos, (long long)n_var);
        if (!out) { std::fputs("\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n", o_.f); return; }
        char b[6][48];
        for (int i = 0; i < 6; ++i) { const double v = out[1 + i]; if (v != v) std::snprintf(b[i], sizeof b[i], "NA"); else std::snprintf(b[i], sizeof b[i], "%.6g", v); }
        const char* st = out[6] != out[6] ? "NA" : (out[7] == 1.0 ? "Y" : (out[7] == 2.0 ? "F" : "N"));
        std::fprintf(o_.f, "\t%lld\t%s\t%s\t%s\t%s\t%s\t%s\t%s\n", (long long)out[0], b[0], b[1], b[2], b[3], b[4], b[5], st);
    }

private:
    OutFile o_;
};

// ---- genotype counts inside sample groups and Fst: the twins of io.read_within, io.align_within, io.group_count_bands,
// io.write_frq_strat, io.write_fst_summary and io.write_fst_var (same rules, same error texts, byte-identical files) ---------------------
constexpr int64_t kGroupsMax = 64;
struct WithinTable {
    std::vector<std::string> family_ids, sample_ids, groups;   // groups: "" = in no group (NA)
    std::vector<uint8_t> has_group;
    std::vector<std::string> names;                              // the group names in order of first appearance in the file
};
// A whitespace-separated table `FID IID GROUP`.  The header (a leading '#' allowed) is required; `NA` means no group; a repeated
// (FID, IID) is refused.
inline WithinTable read_within(const std::string& path) {
    std::ifstream in(path);
    if (!in) throw std::runtime_error("cannot open " + path);
    WithinTable t;
    bool have_header = false;
    std::set<std::pair<std::string, std::string>> seen;
    std::set<std::string> known;
    std::string line;
    const std::string need = path + ": the header `FID IID GROUP` is required";
    auto upper = [](std::string s) { for (char& c : s) c = (char)std::toupper((unsigned char)c); return s; };
    for (int64_t ln = 1; std::getline(in, line); ++ln) {
        const std::vector<std::string> p = split_ws(line);
        if (p.empty()) continue;
        if (!have_header) {
            if (p.size() != 3 || upper(p[0].substr(std::min(p[0].find_first_not_of('#'), p[0].size()))) != "FID" || upper(p[1]) != "IID" ||
                upper(p[2]) != "GROUP")
                throw std::runtime_error(need);
            have_header = true;
            continue;
        }
        const std::string at = path + ":" + std::to_string(ln) + ": ";
        if (p.size() != 3) throw std::runtime_error(at + std::to_string(p.size()) + " fields, the header has 3");
        if (!seen.insert({p[0], p[1]}).second) throw std::runtime_error(at + "sample " + p[0] + " " + p[1] + " appears twice");
        const bool has = p[2] != "NA";
        if (has && known.insert(p[2]).second) t.names.push_back(p[2]);
        t.family_ids.push_back(p[0]); t.sample_ids.push_back(p[1]); t.groups.push_back(has ? p[2] : std::string()); t.has_group.push_back(has ? 1 : 0);
    }
    if (!have_header) throw std::runtime_error(need);
    return t;
}
// labels in .fam order: p = the sample is in group names[p], -1 = it is absent from the table or has no group
inline std::vector<int32_t> align_within(const WithinTable& t, const std::vector<std::string>& family_ids, const std::vector<std::string>& sample_ids) {
    std::map<std::string, int32_t> index;
    for (size_t p = 0; p < t.names.size(); ++p) index[t.names[p]] = (int32_t)p;
    std::map<std::pair<std::string, std::string>, size_t> at;
    for (size_t r = 0; r < t.sample_ids.size(); ++r) at[{t.family_ids[r], t.sample_ids[r]}] = r;
    std::vector<int32_t> out(sample_ids.size(), -1);
    for (size_t n = 0; n < sample_ids.size(); ++n) {
        const auto it = at.find({family_ids[n], sample_ids[n]});
        if (it != at.end() && t.has_group[it->second]) out[n] = index[t.groups[it->second]];
    }
    return out;
}
// [row0, row1) bands of the K kept rows whose counts (rows x P x 3) hold at most max_values entries (at least one row); max_rows > 0: no
// band holds more rows than that (kF2BandRowsMax for gpca_f2_blocks)
constexpr int64_t kF2BandRowsMax = (int64_t)1 << 21;
inline std::vector<std::pair<int64_t, int64_t>> group_count_bands(int64_t K, int64_t P, int64_t max_values = (int64_t)1 << 26, int64_t max_rows = 0) {
    int64_t step = std::max<int64_t>(max_values / (3 * std::max<int64_t>(P, 1)), 1);
    if (max_rows > 0) step = std::max<int64_t>(std::min(step, max_rows), 1);
    std::vector<std::pair<int64_t, int64_t>> out;
    for (int64_t r0 = 0; r0 < K; r0 += step) out.emplace_back(r0, std::min(r0 + step, K));
    return out;
}
inline void fmt_g6(char (&b)[48], double v) { if (v != v) std::snprintf(b, sizeof b, "NA"); else std::snprintf(b, sizeof b, "%.6g", v); }
inline void fmt_ratio6(char (&b)[48], double num, double den) {
    if (num != num || den != den || den == 0.0) std::snprintf(b, sizeof b, "NA"); else fmt_g6(b, num / den);
}
// The stratified frequency file `path` (P.frq.strat, P.<trait>.frq.cc): one tab-separated line per SNP and group, SNP-major, `#CHROM POS
// ID A1 GROUP OBS_CT A1_CT A1_FREQ HET_CT HOM_A1_CT HWE_P` from a SNP's counts [groups][3] = n_obs, n_het, n_hom2; A1_FREQ and HWE_P (the
// caller's function: gpca_hwe_chi_squared_p_value) as %.6g, NA where OBS_CT = 0; rows are added band by band
class FrqStratWriter {
public:
    FrqStratWriter(const std::string& path, const std::vector<std::string>& names, double (*hwe)(uint64_t, uint64_t, uint64_t))
        : o_(path), names_(names), hwe_(hwe) {
        std::fputs("#CHROM\tPOS\tID\tA1\tGROUP\tOBS_CT\tA1_CT\tA1_FREQ\tHET_CT\tHOM_A1_CT\tHWE_P\n", o_.f);
    }
    void add_row(const std::string& chrom, int64_t pos, const std::string& id, const std::string& a1, const uint32_t* counts) {
        for (size_t p = 0; p < names_.size(); ++p) {
            const uint64_t obs = counts[3 * p], het = counts[3 * p + 1], hom = counts[3 * p + 2], ac = het + 2 * hom;
            char fr[48], hw[48];
            if (obs == 0) { fmt_g6(fr, std::nan("")); fmt_g6(hw, std::nan("")); }
            else { fmt_g6(fr, (double)ac / (2.0 * (double)obs)); fmt_g6(hw, hwe_(obs - het - hom, het, hom)); }
            std::fprintf(o_.f, "%s\t%lld\t%s\t%s\t%s\t%llu\t%llu\t%s\t%llu\t%llu\t%s\n", chrom.c_str(), (long long)pos, id.c_str(), a1.c_str(),
                         names_[p].c_str(), (unsigned long long)obs, (unsigned long long)ac, fr, (unsigned long long)het, (unsigned long long)hom, hw);
        }
    }

private:
    OutFile o_;
    std::vector<std::string> names_;
    double (*hwe_)(uint64_t, uint64_t, uint64_t);
};
// P.fst.summary: `#GROUP1 GROUP2 N_VAR HUDSON_FST` (wc = false) or `... WC_FST`, one line per pair (j < i at i (i - 1) / 2 + j, GROUP1 the
// earlier group) from sums [pairs][3]; for wc with more than two groups a further last row of sums is written as `* * N_VAR FST`
inline void write_fst_summary(const std::string& prefix, bool wc, const std::vector<std::string>& names, const std::vector<double>& sums) {
    const size_t P = names.size(), pairs = P * (P - 1) / 2;
    const bool joint = wc && P > 2;
    if (sums.size() != (pairs + (joint ? 1 : 0)) * 3)
        throw std::runtime_error("write_fst_summary: sums must be [pairs][3] (one more row for the joint wc value of more than two groups)");
    OutFile o(prefix + ".fst.summary");
    std::fprintf(o.f, "#GROUP1\tGROUP2\tN_VAR\t%s\n", wc ? "WC_FST" : "HUDSON_FST");
    char b[48];
    size_t q = 0;
    for (size_t i = 1; i < P; ++i)
        for (size_t j = 0; j < i; ++j, ++q) {
            if (sums[3 * q + 2] == 0.0) fmt_g6(b, std::nan("")); else fmt_ratio6(b, sums[3 * q], sums[3 * q + 1]);
            std::fprintf(o.f, "%s\t%s\t%lld\t%s\n", names[j].c_str(), names[i].c_str(), (long long)sums[3 * q + 2], b);
        }
    if (joint) {
        if (sums[3 * q + 2] == 0.0) fmt_g6(b, std::nan("")); else fmt_ratio6(b, sums[3 * q], sums[3 * q + 1]);
        std::fprintf(o.f, "*\t*\t%lld\t%s\n", (long long)sums[3 * q + 2], b);
    }
}
// P.fst.var: one tab-separated line per SNP and pair (SNP-major): `#CHROM POS ID GROUP1 GROUP2 NUM DEN FST` (wc = false; a SNP's values
// [pairs][2] = num, den) or `#CHROM POS ID GROUP1 GROUP2 A B C FST` (values [pairs][3] = a, b, c); %.6g, NaN as NA; FST = NUM / DEN or
// A / ((A + B) + C), NA where that is NaN or the denominator is 0; rows are added band by band
class FstVarWriter {
public:
    FstVarWriter(const std::string& prefix, bool wc, const std::vector<std::string>& names) : o_(prefix + ".fst.var"), wc_(wc), names_(names) {
        std::fprintf(o_.f, "#CHROM\tPOS\tID\tGROUP1\tGROUP2\t%s\tFST\n", wc ? "A\tB\tC" : "NUM\tDEN");
    }
    void add_row(const std::string& chrom, int64_t pos, const std::string& id, const double* values) {
        const int w = wc_ ? 3 : 2;
        size_t q = 0;
        for (size_t i = 1; i < names_.size(); ++i)
            for (size_t j = 0; j < i; ++j, ++q) {
                const double* v = values + q * w;
                char b[4][48];
                for (int k = 0; k < w; ++k) fmt_g6(b[k], v[k]);
                fmt_ratio6(b[3], v[0], wc_ ? (v[0] + v[1]) + v[2] : v[1]);
                std::fprintf(o_.f, "%s\t%lld\t%s\t%s\t%s\t%s\t%s\t", chrom.c_str(), (long long)pos, id.c_str(), names_[j].c_str(), names_[i].c_str(), b[0], b[1]);
                if (wc_) std::fprintf(o_.f, "%s\t", b[2]);
                std::fprintf(o_.f, "%s\n", b[3]);
            }
    }

private:
    OutFile o_;
    bool wc_;
    std::vector<std::string> names_;
};

// ---- f-statistics: the twins of io.fstat_blocks, io.read_fstats_list, io.fstat_quad, io.write_f2_summary and io.write_fstats (same
// rules, same error texts, byte-identical files) ----------------------------------------------------------------------------------------
// block [K] and B: the jackknife block of every SNP of a list in genome order (gpca_fstat_blocks' rule; include/gpca.h section a23).  spec
// has parse_ld_window's grammar: "500" = blocks of 500 variants, "5000kb" = a block ends before the first SNP 5 000 000 bp or more beyond
// its first one; a new block starts at every change of chromosome.
inline std::vector<int32_t> fstat_blocks(const std::vector<std::string>& chromosomes, const std::vector<int64_t>& positions, const std::string& spec,
                                         int32_t& n_blocks) {
    const LdWindow lw = parse_ld_window(spec);
    const size_t K = chromosomes.size();
    if (positions.size() != K) throw std::runtime_error("fstat_blocks: one position per chromosome entry");
    std::vector<int32_t> block(K);
    int64_t b = -1, held = 0, first = 0;
    std::string prev;
    for (size_t r = 0; r < K; ++r) {
        const std::string c = normalize_chromosome_name(chromosomes[r]);
        const bool start = r == 0 || c != prev || (lw.bp ? positions[r] - first >= lw.w : held >= lw.w);
        if (start) { ++b; held = 0; first = positions[r]; }
        block[r] = (int32_t)b;
        ++held;
        prev = c;
    }
    n_blocks = (int32_t)(b + 1);
    return block;
}
struct FstatSpec { std::string kind; std::vector<int32_t> groups; };   // kind: f2, f3 or f4; groups: indices into the within file's names
// The statistics of --gpca-fstats: one per line, `f2 A B`, `f3 C A B` (C is the target) or `f4 A B C D` with group names; '#' lines and
// blank lines are skipped.
inline std::vector<FstatSpec> read_fstats_list(const std::string& path, const std::vector<std::string>& names) {
    std::ifstream in(path);
    if (!in) throw std::runtime_error("cannot open " + path);
    std::map<std::string, int32_t> index;
    for (size_t p = 0; p < names.size(); ++p) index[names[p]] = (int32_t)p;
    std::vector<FstatSpec> out;
    std::string line;
    for (int64_t ln = 1; std::getline(in, line); ++ln) {
        const std::vector<std::string> p = split_ws(line);
        if (p.empty() || p[0][0] == '#') continue;
        const std::string at = path + ":" + std::to_string(ln) + ": ";
        const size_t arity = p[0] == "f2" ? 2 : p[0] == "f3" ? 3 : p[0] == "f4" ? 4 : 0;
        if (arity == 0) throw std::runtime_error(at + "'" + p[0] + "' is not f2, f3 or f4");
        if (p.size() - 1 != arity) throw std::runtime_error(at + p[0] + " takes " + std::to_string(arity) + " groups, " + std::to_string(p.size() - 1) + " are given");
        FstatSpec s;
        s.kind = p[0];
        for (size_t k = 1; k < p.size(); ++k) {
            const auto it = index.find(p[k]);
            if (it == index.end()) throw std::runtime_error(at + "no group '" + p[k] + "' in the within file");
            s.groups.push_back(it->second);
        }
        out.push_back(s);
    }
    return out;
}
// gpca_fstat's quad (a, b, c, d), read as f4(a, b; c, d): f2(A, B) = (A, B, A, B), f3(C; A, B) = (C, A, C, B), f4 as it is
inline void fstat_quad(const FstatSpec& s, int32_t (&q)[4]) {
    const std::vector<int32_t>& g = s.groups;
    if (s.kind == "f2" && g.size() == 2) { q[0] = g[0]; q[1] = g[1]; q[2] = g[0]; q[3] = g[1]; }
    else if (s.kind == "f3" && g.size() == 3) { q[0] = g[0]; q[1] = g[1]; q[2] = g[0]; q[3] = g[2]; }
    else if (s.kind == "f4" && g.size() == 4) { q[0] = g[0]; q[1] = g[1]; q[2] = g[2]; q[3] = g[3]; }
    else throw std::runtime_error("fstat_quad: f2 takes 2 groups, f3 3 and f4 4");
}
inline void fmt_count_or_na(char (&b)[48], double v) { if (v != v) std::snprintf(b, sizeof b, "NA"); else std::snprintf(b, sizeof b, "%lld", (long long)v); }
inline void write_fstat_tail(std::FILE* f, const double* s) {   // EST SE Z N_BLOCKS N_SNPS of one row of gpca_fstat
    char b[5][48];
    fmt_g6(b[0], s[0]); fmt_g6(b[1], s[2]); fmt_g6(b[2], s[3]); fmt_count_or_na(b[3], s[4]); fmt_count_or_na(b[4], s[5]);
    std::fprintf(f, "\t%s\t%s\t%s\t%s\t%s\n", b[0], b[1], b[2], b[3], b[4]);
}
// P.f2.summary: `#POP1 POP2 F2 SE Z N_BLOCKS N_SNPS`, one line per pair (j < i at i (i - 1) / 2 + j, POP1 the earlier group) from stats
// [pairs][6] = gpca_fstat's rows of the quads (j, i, j, i); %.6g, NaN as NA
inline void write_f2_summary(const std::string& prefix, const std::vector<std::string>& names, const std::vector<double>& stats) {
    const size_t P = names.size(), pairs = P * (P - 1) / 2;
    if (stats.size() != pairs * 6) throw std::runtime_error("write_f2_summary: stats must be [pairs][6]");
    OutFile o(prefix + ".f2.summary");
    std::fputs("#POP1\tPOP2\tF2\tSE\tZ\tN_BLOCKS\tN_SNPS\n", o.f);
    size_t q = 0;
    for (size_t i = 1; i < P; ++i)
        for (size_t j = 0; j < i; ++j, ++q) {
            std::fprintf(o.f, "%s\t%s", names[j].c_str(), names[i].c_str());
            write_fstat_tail(o.f, &stats[6 * q]);
        }
}
// P.fstats: `#STAT POP1 POP2 POP3 POP4 EST SE Z N_BLOCKS N_SNPS`, one line per statistic of the list in its order, `.` for the columns a
// statistic does not have; stats [M][6] = gpca_fstat's rows of fstat_quad of each
inline void write_fstats(const std::string& prefix, const std::vector<std::string>& names, const std::vector<FstatSpec>& list,
                         const std::vector<double>& stats) {
    if (stats.size() != list.size() * 6) throw std::runtime_error("write_fstats: one row of stats per statistic");
    OutFile o(prefix + ".fstats");
    std::fputs("#STAT\tPOP1\tPOP2\tPOP3\tPOP4\tEST\tSE\tZ\tN_BLOCKS\tN_SNPS\n", o.f);
    for (size_t m = 0; m < list.size(); ++m) {
        std::fputs(list[m].kind.c_str(), o.f);
        for (size_t k = 0; k < 4; ++k) std::fprintf(o.f, "\t%s", k < list[m].groups.size() ? names[(size_t)list[m].groups[k]].c_str() : ".");
        write_fstat_tail(o.f, &stats[6 * m]);
    }
}

// ---- genotype counts per sample, heterozygosity F and sample QC: the twins of io.sample_count_bands, io.write_smiss, io.write_het,
// io.sample_qc_pass and io.write_sample_qc_ids (same rules, byte-identical files) --------------------------------------------------------
inline std::vector<std::pair<int64_t, int64_t>> sample_count_bands(int64_t K, int64_t max_rows = (int64_t)1 << 24) {
    const int64_t step = std::max<int64_t>(max_rows, 1);
    std::vector<std::pair<int64_t, int64_t>> out;
    for (int64_t r0 = 0; r0 < K; r0 += step) out.emplace_back(r0, std::min(r0 + step, K));
    return out;
}
// P.smiss: `#FID IID MISSING_CT OBS_CT F_MISS` from counts [N][3] over K SNPs: MISSING_CT = K - n_obs, OBS_CT = K, F_MISS as %.6g
inline void write_smiss(const std::string& prefix, const std::vector<std::string>& fids, const std::vector<std::string>& iids,
                        const std::vector<uint32_t>& counts, int64_t K) {
    const size_t n = iids.size();
    if (counts.size() != 3 * n || fids.size() != n) throw std::runtime_error("write_smiss: counts must be [samples][3] with one FID and IID per sample");
    OutFile o(prefix + ".smiss");
    std::fputs("#FID\tIID\tMISSING_CT\tOBS_CT\tF_MISS\n", o.f);
    char b[48];
    for (size_t i = 0; i < n; ++i) {
        const int64_t mis = K - (int64_t)counts[3 * i];
        fmt_g6(b, K == 0 ? std::nan("") : (double)mis / (double)K);
        std::fprintf(o.f, "%s\t%s\t%lld\t%lld\t%s\n", fids[i].c_str(), iids[i].c_str(), (long long)mis, (long long)K, b);
    }
}
// P.het: `#FID IID O_HOM E_HOM OBS_CT F` from counts [N][3] (OBS_CT = n_obs) and het [N][3] = O_HOM, E_HOM, F; %.6g, NaN as NA
inline void write_het(const std::string& prefix, const std::vector<std::string>& fids, const std::vector<std::string>& iids,
                      const std::vector<uint32_t>& counts, const std::vector<double>& het) {
    const size_t n = iids.size();
    if (counts.size() != 3 * n || het.size() != 3 * n || fids.size() != n)
        throw std::runtime_error("write_het: counts and het must be [samples][3] with one FID and IID per sample");
    OutFile o(prefix + ".het");
    std::fputs("#FID\tIID\tO_HOM\tE_HOM\tOBS_CT\tF\n", o.f);
    char b[3][48];
    for (size_t i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) fmt_g6(b[k], het[3 * i + k]);
        std::fprintf(o.f, "%s\t%s\t%s\t%s\t%llu\t%s\n", fids[i].c_str(), iids[i].c_str(), b[0], b[1], (unsigned long long)counts[3 * i], b[2]);
    }
}
// The sample filters: pass [N] and reason [N] (kSampleQcNone, kSampleQcMind, kSampleQcHet) from counts [N][3] over K SNPs and F [N]
// (read with het_sd).  Sequential f64 loops in sample order:
//   mind:   F_MISS = (K - n_obs) / K; a sample fails MIND if n_obs = 0 or F_MISS > mind.
//   het_sd: over the c samples that pass MIND and have a finite F, m = (sum F) / c and s = sqrt(sum (F - m)^2 / (c - 1)); a sample that
//           passes MIND fails HET if F is NaN or |F - m| > het_sd s.  One round; with c < 2 or s = 0 only NaN fails.
constexpr uint8_t kSampleQcNone = 0, kSampleQcMind = 1, kSampleQcHet = 2;
inline void sample_qc_pass(const std::vector<uint32_t>& counts, int64_t K, const std::vector<double>& F, bool use_mind, double mind,
                           bool use_het, double het_sd, std::vector<uint8_t>& pass, std::vector<uint8_t>& reason) {
    const size_t n = counts.size() / 3;
    if (counts.size() != 3 * n) throw std::runtime_error("sample_qc_pass: counts must be [samples][3]");
    pass.assign(n, 1); reason.assign(n, kSampleQcNone);
    if (use_mind)
        for (size_t i = 0; i < n; ++i) {
            const int64_t nobs = counts[3 * i];
            if (nobs == 0 || (double)(K - nobs) / (double)K > mind) { pass[i] = 0; reason[i] = kSampleQcMind; }
        }
    if (use_het) {
        if (F.size() != n) throw std::runtime_error("sample_qc_pass: het_sd needs F with one entry per sample");
        int64_t c = 0;
        double tot = 0.0;
        for (size_t i = 0; i < n; ++i)
            if (pass[i] && std::isfinite(F[i])) { ++c; tot = tot + F[i]; }
        const double m = c ? tot / (double)c : 0.0;
        double ss = 0.0;
        for (size_t i = 0; i < n; ++i)
            if (pass[i] && std::isfinite(F[i])) { const double d = F[i] - m; ss = ss + d * d; }
        const double s = c >= 2 ? std::sqrt(ss / (double)(c - 1)) : 0.0;
        for (size_t i = 0; i < n; ++i) {
            if (!pass[i]) continue;
            const double x = F[i];
            if (x != x || (c >= 2 && s > 0.0 && std::fabs(x - m) > het_sd * s)) { pass[i] = 0; reason[i] = kSampleQcHet; }
        }
    }
}
// P.sampleqc.in.id (`#FID IID`) and P.sampleqc.out.id (`#FID IID REASON`, MIND or HET), in sample order
inline void write_sample_qc_ids(const std::string& prefix, const std::vector<std::string>& fids, const std::vector<std::string>& iids,
                                const std::vector<uint8_t>& pass, const std::vector<uint8_t>& reason) {
    const size_t n = iids.size();
    if (fids.size() != n || pass.size() != n || reason.size() != n) throw std::runtime_error("write_sample_qc_ids: one entry per sample in every column");
    OutFile in(prefix + ".sampleqc.in.id"), out(prefix + ".sampleqc.out.id");
    std::fputs("#FID\tIID\n", in.f);
    std::fputs("#FID\tIID\tREASON\n", out.f);
    for (size_t i = 0; i < n; ++i) {
        if (pass[i]) std::fprintf(in.f, "%s\t%s\n", fids[i].c_str(), iids[i].c_str());
        else std::fprintf(out.f, "%s\t%s\t%s\n", fids[i].c_str(), iids[i].c_str(), reason[i] == kSampleQcMind ? "MIND" : reason[i] == kSampleQcHet ? "HET" : "None");
    }
}

// ---- runs of homozygosity: the twins of io.roh_breaks, io.roh_bands, io.roh_select, io.roh_summary and io.write_hom (same rules,
// byte-identical files) ---------------------------------------------------------------------------------------------------------------------
// brk [K] over the kept SNPs, in their order: 3 at the first SNP of every chromosome run, 2 at a SNP more than max_gap_bp behind the SNP
// before it, else 0
inline std::vector<uint8_t> roh_breaks(const std::vector<std::string>& chromosomes, const std::vector<int64_t>& positions, int64_t max_gap_bp) {
    const int64_t K = (int64_t)chromosomes.size();
    if ((int64_t)positions.size() != K) throw std::runtime_error("roh_breaks: one position per chromosome entry");
    if (max_gap_bp < 0) throw std::runtime_error("roh_breaks: the gap must be at least 0");
    std::vector<uint8_t> brk((size_t)K, 0);
    std::set<std::string> seen;
    for (int64_t s = 0; s < K;) {
        const std::string c = normalize_chromosome_name(chromosomes[(size_t)s]);
        if (!seen.insert(c).second)
            throw std::runtime_error("roh_breaks: chromosome '" + chromosomes[(size_t)s] + "' reappears at variant " + std::to_string(s) +
                                     " after another chromosome: sort the variants");
        brk[(size_t)s] = 3;
        int64_t e = s + 1;
        while (e < K && normalize_chromosome_name(chromosomes[(size_t)e]) == c) {
            if (positions[(size_t)e] < positions[(size_t)e - 1])
                throw std::runtime_error("roh_breaks: the position of variant " + std::to_string(e) + " (" + std::to_string(positions[(size_t)e]) +
                                         ") is below that of the variant before it on chromosome '" + chromosomes[(size_t)e] + "': sort the variants");
            if (positions[(size_t)e] - positions[(size_t)e - 1] > max_gap_bp) brk[(size_t)e] = 2;
            ++e;
        }
        s = e;
    }
    return brk;
}
// the first rows of the window domains of brk (row 0 starts one), then K
inline std::vector<int64_t> roh_domain_starts(const std::vector<uint8_t>& brk) {
    std::vector<int64_t> starts{0};
    for (size_t j = 1; j < brk.size(); ++j) if (brk[j] & 1u) starts.push_back((int64_t)j);
    starts.push_back((int64_t)brk.size());
    return starts;
}
// [row0, row1) bands cut only where a domain starts: whole domains are added while the band stays within max_rows rows
inline std::vector<std::pair<int64_t, int64_t>> roh_bands(const std::vector<uint8_t>& brk, int64_t max_rows = (int64_t)1 << 24) {
    const std::vector<int64_t> starts = roh_domain_starts(brk);
    std::vector<std::pair<int64_t, int64_t>> out;
    int64_t r0 = 0;
    for (size_t d = 1; d < starts.size(); ++d) {
        if (d + 1 < starts.size() && starts[d + 1] - r0 <= std::max<int64_t>(max_rows, 1)) continue;
        if (starts[d] > r0) out.emplace_back(r0, starts[d]);
        r0 = starts[d];
    }
    return out;
}
// keep [n] of the records segs [n][5] by length and density (gpca_roh_select's rule, in integers)
inline std::vector<uint8_t> roh_select(const std::vector<uint32_t>& segs, const std::vector<int64_t>& positions, int64_t min_bp, int64_t max_bp_per_snp) {
    const size_t n = segs.size() / 5;
    std::vector<uint8_t> keep(n, 0);
    for (size_t i = 0; i < n; ++i) {
        const int64_t first = segs[5 * i + 1], last = segs[5 * i + 2];
        if (last < first) throw std::runtime_error("roh_select: record " + std::to_string(i) + " ends before it starts");
        const int64_t span = positions[(size_t)last] - positions[(size_t)first], nsnp = last - first + 1;
        keep[i] = (span >= min_bp && span / nsnp + (span % nsnp != 0 ? 1 : 0) <= max_bp_per_snp) ? 1 : 0;
    }
    return keep;
}
// per sample, from the kept records: NSEG, total bp and FROH = total bp / (the sum over the domains of pos[last row] - pos[first row]),
// NaN when that sum is 0
inline void roh_summary(const std::vector<uint32_t>& segs, const std::vector<uint8_t>& keep, const std::vector<int64_t>& positions,
                        const std::vector<uint8_t>& brk, size_t n_samples, std::vector<int64_t>& nseg, std::vector<int64_t>& total,
                        std::vector<double>& froh) {
    const size_t n = segs.size() / 5;
    if (keep.size() != n || positions.size() != brk.size()) throw std::runtime_error("roh_summary: one keep flag per record and one position per row of brk");
    const std::vector<int64_t> starts = roh_domain_starts(brk);
    int64_t genome = 0;
    for (size_t d = 0; d + 1 < starts.size(); ++d)
        if (starts[d + 1] > starts[d]) genome += positions[(size_t)starts[d + 1] - 1] - positions[(size_t)starts[d]];
    nseg.assign(n_samples, 0); total.assign(n_samples, 0); froh.assign(n_samples, std::nan(""));
    for (size_t i = 0; i < n; ++i)
        if (keep[i]) { nseg[segs[5 * i]] += 1; total[segs[5 * i]] += positions[segs[5 * i + 2]] - positions[segs[5 * i + 1]]; }
    if (genome > 0) for (size_t s = 0; s < n_samples; ++s) froh[s] = (double)total[s] / (double)genome;
}
// P.hom: `#FID IID CHROM SNP1 SNP2 POS1 POS2 KB NSNP DENSITY PHOM PHET`, one line per kept record; P.hom.indiv: `#FID IID NSEG KB KBAVG FROH`
inline void write_hom(const std::string& prefix, const std::vector<std::string>& fids, const std::vector<std::string>& iids,
                      const std::vector<std::string>& chromosomes, const std::vector<std::string>& variant_ids, const std::vector<int64_t>& positions,
                      const std::vector<uint32_t>& segs, const std::vector<uint8_t>& keep, const std::vector<uint8_t>& brk) {
    const size_t n = iids.size(), nrec = segs.size() / 5;
    if (fids.size() != n || keep.size() != nrec || chromosomes.size() != positions.size() || variant_ids.size() != positions.size())
        throw std::runtime_error("write_hom: one FID per IID, one keep flag per record, one chromosome and id per position");
    std::vector<int64_t> nseg, total;
    std::vector<double> froh;
    roh_summary(segs, keep, positions, brk, n, nseg, total, froh);
    char b[4][48];
    {
        OutFile o(prefix + ".hom");
        std::fputs("#FID\tIID\tCHROM\tSNP1\tSNP2\tPOS1\tPOS2\tKB\tNSNP\tDENSITY\tPHOM\tPHET\n", o.f);
        for (size_t i = 0; i < nrec; ++i) {
            if (!keep[i]) continue;
            const size_t s = segs[5 * i], first = segs[5 * i + 1], last = segs[5 * i + 2];
            const int64_t nsnp = (int64_t)last - (int64_t)first + 1, nh = segs[5 * i + 3], nm = segs[5 * i + 4];
            const double kb = (double)(positions[last] - positions[first]) / 1000.0;
            fmt_g6(b[0], kb); fmt_g6(b[1], kb / (double)nsnp); fmt_g6(b[2], (double)(nsnp - nh - nm) / (double)nsnp); fmt_g6(b[3], (double)nh / (double)nsnp);
            std::fprintf(o.f, "%s\t%s\t%s\t%s\t%s\t%lld\t%lld\t%s\t%lld\t%s\t%s\t%s\n", fids[s].c_str(), iids[s].c_str(), chromosomes[first].c_str(),
                         variant_ids[first].c_str(), variant_ids[last].c_str(), (long long)positions[first], (long long)positions[last], b[0],
                         (long long)nsnp, b[1], b[2], b[3]);
        }
    }
    OutFile o(prefix + ".hom.indiv");
    std::fputs("#FID\tIID\tNSEG\tKB\tKBAVG\tFROH\n", o.f);
    for (size_t i = 0; i < n; ++i) {
        const double kb = (double)total[i] / 1000.0;
        fmt_g6(b[0], kb); fmt_g6(b[1], nseg[i] == 0 ? std::nan("") : kb / (double)nseg[i]); fmt_g6(b[2], froh[i]);
        std::fprintf(o.f, "%s\t%s\t%lld\t%s\t%s\t%s\n", fids[i].c_str(), iids[i].c_str(), (long long)nseg[i], b[0], b[1], b[2]);
    }
}
// ---- admixture proportions (gpca_admix; gpca.h section a21): the host rules around the fit; twins of io.admix_order, io.admix_supervised
// and io.write_admix
// the column order: by descending column sum of Q [n][K] over the samples with mode != 1 (f64, sample order), ties to the lower index;
// the identity with a mode-1 sample
inline std::vector<int64_t> admix_order(const std::vector<float>& Q, size_t n, int K, const std::vector<uint8_t>& mode) {
    std::vector<int64_t> order((size_t)K);
    for (int k = 0; k < K; ++k) order[(size_t)k] = k;
    for (size_t s = 0; s < n && s < mode.size(); ++s)
        if (mode[s] == 1) return order;
    std::vector<double> sums((size_t)K, 0.0);
    for (size_t s = 0; s < n; ++s)
        for (int k = 0; k < K; ++k) sums[(size_t)k] += (double)Q[s * (size_t)K + (size_t)k];
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return sums[(size_t)a] > sums[(size_t)b]; });
    return order;
}
// a labelled sample's row of Q [n][K] becomes the one-hot row of its group, clamped to >= 1e-5 and divided by its sum (f32, columns
// ascending), and its mode 1; an unlabelled sample (label < 0) keeps its row and mode 0
inline std::vector<uint8_t> admix_supervised(const std::vector<int32_t>& labels, int K, std::vector<float>& Q) {
    std::vector<uint8_t> mode(labels.size(), 0);
    for (size_t s = 0; s < labels.size(); ++s) {
        if (labels[s] < 0) continue;
        mode[s] = 1;
        float* row = Q.data() + s * (size_t)K;
        float sum = 0.0f;
        for (int k = 0; k < K; ++k) { row[k] = k == labels[s] ? 1.0f : 1e-5f; sum = sum + row[k]; }
        const float d = sum;
        for (int k = 0; k < K; ++k) row[k] = row[k] / d;
    }
    return mode;
}
// P.K.Q and P.K.P: K `%.6f` per line, separated by spaces, columns in `order`; P.K.Q.id: `#FID IID`; P.K.P.id: one variant id per line;
// P.K.admix.log: `#K SEED STEPS CYCLES CONVERGED LOGLIK`
inline void write_admix(const std::string& prefix, int K, const std::vector<std::string>& fids, const std::vector<std::string>& iids,
                        const std::vector<std::string>& variant_ids, const std::vector<float>& Q, const std::vector<float>& F,
                        const std::vector<int64_t>& order, uint64_t seed, int64_t steps, int64_t cycles, bool converged, double loglik) {
    if (fids.size() != iids.size() || Q.size() != iids.size() * (size_t)K || F.size() != variant_ids.size() * (size_t)K || order.size() != (size_t)K)
        throw std::runtime_error("write_admix: Q must be [samples][K] and F [SNPs][K], with one FID per IID");
    const std::string base = prefix + "." + std::to_string(K);
    auto matrix = [&](const std::string& path, const std::vector<float>& m, size_t rows) {
        OutFile o(path);
        for (size_t i = 0; i < rows; ++i)
            for (int k = 0; k < K; ++k) std::fprintf(o.f, k + 1 < K ? "%.6f " : "%.6f\n", (double)m[i * (size_t)K + (size_t)order[(size_t)k]]);
    };
    matrix(base + ".Q", Q, iids.size());
    matrix(base + ".P", F, variant_ids.size());
    {
        OutFile o(base + ".Q.id");
        std::fputs("#FID\tIID\n", o.f);
        for (size_t i = 0; i < iids.size(); ++i) std::fprintf(o.f, "%s\t%s\n", fids[i].c_str(), iids[i].c_str());
    }
    {
        OutFile o(base + ".P.id");
        for (const std::string& v : variant_ids) std::fprintf(o.f, "%s\n", v.c_str());
    }
    OutFile o(base + ".admix.log");
    std::fputs("#K\tSEED\tSTEPS\tCYCLES\tCONVERGED\tLOGLIK\n", o.f);
    std::fprintf(o.f, "%d\t%llu\t%lld\t%lld\t%d\t%.4f\n", K, (unsigned long long)seed, (long long)steps, (long long)cycles, converged ? 1 : 0, loglik);
}
// P.admix.cv (io.write_admix_cv; gpca.h section a22): `#K FOLDS CV_SEED FOLD STEPS CONVERGED N_HELD DEVIANCE CV_ERROR`; one line per fold
// (the folds of one K together, ascending; CV_ERROR = deviance / n_held), then per K one line with FOLD `*` and the totals; `%.6f`, NaN as NA
struct AdmixCvRow { int K, folds; uint64_t cv_seed; int fold; int64_t steps; bool converged; int64_t n_held; double deviance; };
inline void write_admix_cv(const std::string& prefix, const std::vector<AdmixCvRow>& rows) {
    OutFile o(prefix + ".admix.cv");
    std::fputs("#K\tFOLDS\tCV_SEED\tFOLD\tSTEPS\tCONVERGED\tN_HELD\tDEVIANCE\tCV_ERROR\n", o.f);
    auto num = [](char* b, size_t n, double x) { if (x != x) std::snprintf(b, n, "NA"); else std::snprintf(b, n, "%.6f", x); };
    auto line = [&](const AdmixCvRow& r, bool total) {
        char fold[16], dev[64], cv[64];
        if (total) std::snprintf(fold, sizeof fold, "*"); else std::snprintf(fold, sizeof fold, "%d", r.fold);
        num(dev, sizeof dev, r.deviance);
        num(cv, sizeof cv, r.n_held > 0 ? r.deviance / (double)r.n_held : std::nan(""));
        std::fprintf(o.f, "%d\t%d\t%llu\t%s\t%lld\t%d\t%lld\t%s\t%s\n", r.K, r.folds, (unsigned long long)r.cv_seed, fold, (long long)r.steps,
                     r.converged ? 1 : 0, (long long)r.n_held, dev, cv);
    };
    for (size_t i = 0; i < rows.size();) {
        size_t j = i;
        AdmixCvRow t = rows[i];
        t.steps = 0; t.converged = true; t.n_held = 0; t.deviance = 0.0;
        for (; j < rows.size() && rows[j].K == rows[i].K; ++j) {
            line(rows[j], false);
            t.steps += rows[j].steps; t.converged = t.converged && rows[j].converged; t.n_held += rows[j].n_held; t.deviance += rows[j].deviance;
        }
        line(t, true);
        i = j;
    }
}
// the threshold of --gpca-homozyg-window-threshold as the exact fraction of its decimal text (digits, one optional point, no exponent),
// reduced; false when the text is not such a number or the reduced denominator is above 2^20 (io / engine: Fraction(str(x)))
inline bool roh_threshold(const std::string& text, int64_t& num, int64_t& den) {
    size_t i = 0;
    __int128 n = 0, d = 1;
    bool point = false, any = false;
    for (; i < text.size(); ++i) {
        const char c = text[i];
        if (c == '.' && !point) { point = true; continue; }
        if (c < '0' || c > '9') return false;
        any = true;
        n = n * 10 + (c - '0');
        if (point) d *= 10;
        if (d > (__int128)1 << 100 || n > (__int128)1 << 100) return false;          // (before either can pass 2^127)
    }
    if (!any) return false;
    __int128 a = n, b = d;
    while (b) { const __int128 t = a % b; a = b; b = t; }
    if (a > 1) { n /= a; d /= a; }
    if (d > ((__int128)1 << 20) || n > ((__int128)1 << 30)) return false;
    num = (int64_t)n; den = (int64_t)d;
    return true;
}

}  // namespace gpca_host

#endif
