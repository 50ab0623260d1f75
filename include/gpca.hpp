/* gpca.hpp -- C++17 host mirror of the reference's operator interface over the C ABI of libgpca.so (gpca.h).
 *
 * Header only; nothing here touches the device except through gpca.h.  The names, argument meaning and error behaviour
 * follow the reference's Rust types at the L2 boundary, so that a host written against them reads the same:
 *
 *   MicroarrayGenotypeAccessor  : impl PcaReadyGenotypeAccessor      /root/reference/src/prepare.rs:1770-1779, 1838-2030
 *   PcaSnpId / QcSampleId       : dense 0-based ids                   /root/reference/src/prepare.rs:1485, 1854, 1858
 *   LdBlockSpecification        :                                     /root/reference/src/prepare.rs:1540-1543
 *   EigenSNPCoreAlgorithmConfig : the 14 fields                       /root/reference/src/main.rs:311-327
 *   EigenSNPCoreAlgorithm       : ::new(cfg).compute_pca(&acc, &blk)  /root/reference/src/main.rs:359-366
 *   PCA                         : ::new / rfit / transform            /root/reference/src/main.rs:602, 648-660
 *
 * Errors: every failed C call becomes a gpca::Error carrying the integer status and the handle's message (the reference
 * returns Result<_, Box<dyn Error + Send + Sync>> with a human string, prepare.rs:61, 1879-1881).
 */
#ifndef GPCA_HPP
#define GPCA_HPP

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "gpca.h"

namespace gpca {

class Error : public std::runtime_error {
public:
    Error(int status, const std::string& msg) : std::runtime_error("[gpca status " + std::to_string(status) + "] " + msg), status_(status) {}
    int status() const { return status_; }
private:
    int status_;
};

using PcaSnpId = int64_t;     // index into the post-QC SNP list   (prepare.rs:1485)
using QcSampleId = int64_t;   // index into the QC'd sample list   (prepare.rs:1854)

struct QcConfig {             // clap's effective defaults with --eigensnp (main.rs:545-560)
    double min_snp_call_rate_threshold = 0.98;
    double min_snp_maf_threshold = 0.01;
    double max_snp_hwe_p_value_threshold = 1e-6;
    static QcConfig none() { return QcConfig{0.0, 0.0, 1.0}; }
};

struct SnpStats { std::vector<float> mu, sigma; std::vector<uint8_t> keep; };

/* One opaque gpca_handle: one GPU, one SNP-row shard of the genotype matrix. */
class Engine {
public:
    explicit Engine(int device = -1, int precision = GPCA_PREC_I8_EXACT, int storage = GPCA_STORE_INT8, int digit_planes = 0)
        : device_(device), precision_(precision), storage_(storage), digit_planes_(digit_planes) {
        gpca_config cfg{};
        cfg.device = device; cfg.precision = precision; cfg.storage = storage; cfg.digit_planes = digit_planes;
        const int rc = gpca_create(&cfg, &h_);
        if (rc != GPCA_OK) throw Error(rc, gpca_last_error(nullptr));
    }
    ~Engine() { if (h_) gpca_destroy(h_); }
    Engine(const Engine&) = delete;
    Engine& operator=(const Engine&) = delete;
    Engine(Engine&& o) noexcept : h_(o.h_), k_(o.k_), device_(o.device_), precision_(o.precision_), storage_(o.storage_), digit_planes_(o.digit_planes_) { o.h_ = nullptr; }

    gpca_handle* handle() const { return h_; }
    void check(int rc) const { if (rc != GPCA_OK) throw Error(rc, gpca_last_error(h_)); }

    /* residency */
    void upload_genotypes_i8(const int8_t* snp_major, int64_t M, int64_t N, int64_t ld) { check(gpca_upload_genotypes_i8(h_, snp_major, M, N, ld)); }
    void upload_bed2bit(const uint8_t* bed_rows, int64_t M, int64_t N) { check(gpca_upload_bed2bit(h_, bed_rows, M, N)); }
    void load_from_source(const gpca_panel_source& src, int64_t M, int64_t N) { check(gpca_load_from_source(h_, &src, M, N)); }
    /* out of core: see gpca.h (gpca_stream_open / _set_fused / _set_cache) */
    void stream_open(const gpca_panel_source& src, int64_t M, int64_t N, int64_t panel_rows = 0, int ring_slots = 3, bool fused = true,
                     int64_t cache_bytes = 0) {
        check(gpca_stream_open(h_, &src, M, N, panel_rows, ring_slots));
        check(gpca_stream_set_fused(h_, fused ? 1 : 0));
        if (cache_bytes != 0) check(gpca_stream_set_cache(h_, cache_bytes, nullptr));
    }
    std::pair<int64_t, int64_t> device_memory() const { int64_t f = 0, t = 0; check(gpca_get_device_memory(h_, &f, &t)); return {f, t}; }   // (free, total) bytes
    std::pair<int64_t, int64_t> dims() const { int64_t M = 0, N = 0; check(gpca_dims(h_, &M, &N)); return {M, N}; }

    /* a1/a3 */
    SnpStats snp_stats(const QcConfig& qc, bool fetch = true) {
        const gpca_qc_config c{qc.min_snp_call_rate_threshold, qc.min_snp_maf_threshold, qc.max_snp_hwe_p_value_threshold};
        SnpStats st;
        if (!fetch) { check(gpca_snp_stats(h_, &c, nullptr, nullptr, nullptr)); return st; }
        const int64_t M = dims().first;
        st.mu.resize((size_t)M); st.sigma.resize((size_t)M); st.keep.resize((size_t)M);
        check(gpca_snp_stats(h_, &c, st.mu.data(), st.sigma.data(), st.keep.data()));
        return st;
    }
    SnpStats get_standardization() const {
        SnpStats st; const int64_t M = dims().first;
        st.mu.resize((size_t)M); st.sigma.resize((size_t)M); st.keep.resize((size_t)M);
        check(gpca_get_standardization(h_, st.mu.data(), st.sigma.data(), st.keep.data()));
        return st;
    }
    void set_standardization(const std::vector<float>& mu, const std::vector<float>& sigma, const std::vector<uint8_t>& keep) {
        const size_t M = (size_t)dims().first;
        if (mu.size() != M || sigma.size() != M || keep.size() != M) throw std::invalid_argument("set_standardization: need one entry per SNP row");
        check(gpca_set_standardization(h_, mu.data(), sigma.data(), keep.data()));
    }
    // counts [M][4] = n_valid, n_hom0, n_het, n_hom2 of the last QC pass (gpca_get_snp_qc_detail)
    std::vector<uint32_t> snp_qc_counts() const {
        std::vector<uint32_t> c(4 * (size_t)dims().first);
        check(gpca_get_snp_qc_detail(h_, c.data(), nullptr));
        return c;
    }
    int64_t num_pca_snps() const { return gpca_num_pca_snps(h_); }
    int64_t num_qc_samples() const { return gpca_num_qc_samples(h_); }
    std::vector<int64_t> pca_snp_rows() const {
        std::vector<int64_t> r((size_t)std::max<int64_t>(num_pca_snps(), 0));
        if (!r.empty()) check(gpca_get_pca_snp_rows(h_, r.data()));
        return r;
    }

    /* a2: the pull API (prepare.rs:1839-2022); out is [snps x samples], C order */
    std::vector<float> standardize_block(const std::vector<PcaSnpId>& snps, const std::vector<QcSampleId>& samples) const {
        std::vector<float> out(snps.size() * samples.size());
        check(gpca_standardize_block(h_, snps.data(), (int64_t)snps.size(), samples.data(), (int64_t)samples.size(), out.data()));
        return out;
    }

    /* f3: the stages of EigenSNPCoreAlgorithm (gpca.h) */
    int device() const { return device_; }
    int precision() const { return precision_; }
    int storage() const { return storage_; }
    int digit_planes() const { return digit_planes_; }
    void copy_rows_from(const Engine& src, int64_t row0, int64_t rows) { check(gpca_copy_rows(h_, src.h_, row0, rows)); }
    void set_sample_mask(const std::vector<uint8_t>* mask) {
        if (mask && (int64_t)mask->size() != dims().second) throw std::invalid_argument("set_sample_mask: one entry per sample");
        check(gpca_set_sample_mask(h_, mask ? mask->data() : nullptr));
    }
    void set_condensed_basis(const std::vector<float>& W, const std::vector<int32_t>& feat0, int cmax, int64_t R) {
        const size_t M = (size_t)dims().first;
        if (feat0.size() != M || W.size() != M * (size_t)cmax) throw std::invalid_argument("set_condensed_basis: W is [SNPs][cmax], feat0 [SNPs]");
        check(gpca_set_condensed_basis(h_, W.data(), feat0.data(), cmax, R));
    }
    void rsvd_condensed(int k, int oversample, int power_iters, uint64_t seed) { check(gpca_rsvd_condensed(h_, k, oversample, power_iters, seed)); k_ = k; }
    void refine(const std::vector<double>& scores, int k) {
        if ((int64_t)scores.size() != dims().second * (int64_t)k) throw std::invalid_argument("refine: scores are [samples][k]");
        check(gpca_refine(h_, scores.data(), k)); k_ = k;
    }

    /* a5/a6 */
    void rsvd(int k, int oversample, int power_iters, uint64_t seed) { check(gpca_rsvd(h_, k, oversample, power_iters, seed)); k_ = k; }
    int components() const { return k_; }
    std::vector<float> scores() const { std::vector<float> s((size_t)num_qc_samples() * (size_t)k_); check(gpca_get_scores(h_, s.data())); return s; }
    std::vector<double> eigenvalues() const { std::vector<double> e((size_t)k_); check(gpca_get_eigenvalues(h_, e.data())); return e; }
    std::vector<float> loadings() const { std::vector<float> l((size_t)num_pca_snps() * (size_t)k_); check(gpca_get_loadings(h_, l.data())); return l; }
    std::vector<double> scores_f64() const { std::vector<double> s((size_t)num_qc_samples() * (size_t)k_); check(gpca_get_scores_f64(h_, s.data())); return s; }
    std::vector<double> transform() const { std::vector<double> s((size_t)num_qc_samples() * (size_t)k_); check(gpca_transform(h_, s.data())); return s; }
    // scores [N][k] of this handle's genotypes on a model (mu, sigma [M], W [M][k]); used (may be null) receives n_used [N]
    std::vector<double> project(const float* mu, const float* sigma, const float* W, int k, std::vector<int32_t>* used = nullptr) const {
        std::vector<double> s((size_t)num_qc_samples() * (size_t)k);
        if (used) used->assign((size_t)num_qc_samples(), 0);
        check(gpca_project(h_, mu, sigma, W, k, s.data(), used ? used->data() : nullptr));
        return s;
    }
    // rows [row0, row1) of the lower triangle of the GRM of the kept rows, packed row-major (gpca_grm); npairs (may be null) receives
    // the number of kept rows where both samples are observed
    std::vector<double> grm(int scaling, int64_t row0, int64_t row1, std::vector<float>* npairs = nullptr) const {
        const size_t e = row1 > row0 ? (size_t)(row1 * (row1 + 1) / 2 - row0 * (row0 + 1) / 2) : 0;
        std::vector<double> g(std::max<size_t>(e, 1));
        if (npairs) npairs->assign(std::max<size_t>(e, 1), 0.f);
        check(gpca_grm(h_, scaling, row0, row1, g.data(), npairs ? npairs->data() : nullptr));
        g.resize(e);
        if (npairs) npairs->resize(e);
        return g;
    }
    // rows [row0, row1) of the strictly lower triangle of the KING-robust kinship of the kept rows, packed row-major (gpca_king); counts
    // (may be null) receives NSNP, HETHET, IBS0 per pair
    std::vector<double> king(int64_t row0, int64_t row1, std::vector<int32_t>* counts = nullptr) const {
        const size_t e = row1 > row0 ? (size_t)(row1 * (row1 - 1) / 2 - row0 * (row0 - 1) / 2) : 0;
        std::vector<double> k(std::max<size_t>(e, 1));
        if (counts) counts->assign(3 * std::max<size_t>(e, 1), 0);
        check(gpca_king(h_, row0, row1, k.data(), counts ? counts->data() : nullptr));
        k.resize(e);
        if (counts) counts->resize(3 * e);
        return k;
    }
    // windowed LD of kept rows [row0, row1) (gpca_ld_window): win_end has one entry per row of the band.  Each output that is not null
    // is resized: r2 [rows][wmax], counts [rows][wmax][6], above [rows][(wmax + 63) / 64] (r2 > threshold); not all three may be null
    void ld_window(int64_t row0, int64_t row1, const std::vector<int64_t>& win_end, int32_t wmax, double threshold, std::vector<double>* r2,
                   std::vector<int32_t>* counts = nullptr, std::vector<uint64_t>* above = nullptr) const {
        const size_t rows = row1 > row0 ? (size_t)(row1 - row0) : 0, w = (size_t)std::max<int32_t>(wmax, 1);
        if (win_end.size() != rows) throw std::invalid_argument("gpca::Engine::ld_window: win_end needs one entry per row of the band");
        if (r2) r2->assign(std::max<size_t>(rows * w, 1), 0.0);
        if (counts) counts->assign(std::max<size_t>(6 * rows * w, 1), 0);
        if (above) above->assign(std::max<size_t>(rows * ((w + 63) / 64), 1), 0);
        check(gpca_ld_window(h_, row0, row1, win_end.data(), wmax, threshold, r2 ? r2->data() : nullptr, counts ? counts->data() : nullptr,
                             above ? above->data() : nullptr));
        if (r2) r2->resize(rows * w);
        if (counts) counts->resize(6 * rows * w);
        if (above) above->resize(rows * ((w + 63) / 64));
    }
    // LD scores of kept rows [row0, row1) from the windowed-LD sweep (gpca_ld_score; gpca.h section a19): score [span] in units of 2^-40
    // and (when not null) partners [span], span = min(K, row1 + wmax) - row0 entries from row0.  WRITTEN per call: the caller adds its bands
    void ld_score(int64_t row0, int64_t row1, const std::vector<int64_t>& win_end, int32_t wmax, bool unbiased, std::vector<int64_t>& score,
                  std::vector<int32_t>* partners = nullptr) const {
        const size_t rows = row1 > row0 ? (size_t)(row1 - row0) : 0;
        if (win_end.size() != rows) throw std::invalid_argument("gpca::Engine::ld_score: win_end needs one entry per row of the band");
        const int64_t K = gpca_num_pca_snps(h_);
        const size_t span = rows ? (size_t)std::max<int64_t>(std::min<int64_t>(K, row1 + std::max<int32_t>(wmax, 0)) - row0, 0) : 0;
        score.assign(std::max<size_t>(span, 1), 0);
        if (partners) partners->assign(std::max<size_t>(span, 1), 0);
        check(gpca_ld_score(h_, row0, row1, win_end.data(), wmax, unbiased ? GPCA_LDSCORE_UNBIASED : 0, score.data(), partners ? partners->data() : nullptr));
        score.resize(span);
        if (partners) partners->resize(span);
    }
    // L2 = 1 + acc 2^-40 of every SNP (gpca_ld_score_total; host only)
    static std::vector<double> ld_score_total(const std::vector<int64_t>& acc) {
        std::vector<double> l2(std::max<size_t>(acc.size(), 1), 0.0);
        const int rc = acc.empty() ? GPCA_OK : gpca_ld_score_total(acc.data(), (int64_t)acc.size(), l2.data());
        if (rc != GPCA_OK) throw Error(rc, std::string("gpca_ld_score_total: ") + gpca_status_string(rc));
        l2.resize(acc.size());
        return l2;
    }
    // LD-score regression (gpca_ldsc_fit; host only; the rule is written out in gpca.h section a19): out [10] = m_used, mean chi2, lambda_GC,
    // intercept, its se, h2, its se, ratio, its se, blocks; w_ell null = ell; chi2_max 0 = no cap
    static std::vector<double> ldsc_fit(const std::vector<double>& chi2, const std::vector<double>& ell, double n_samples, double M,
                                        const std::vector<double>* w_ell = nullptr, int32_t n_blocks = 200, double chi2_max = 0.0) {
        std::vector<double> out(10, 0.0);
        static const double none = 0.0;
        const bool sizes = ell.size() == chi2.size() && (!w_ell || w_ell->size() == chi2.size());
        const int rc = !sizes ? GPCA_ERR_BAD_ARG
                              : gpca_ldsc_fit(chi2.empty() ? &none : chi2.data(), chi2.empty() ? &none : ell.data(),
                                              w_ell ? (chi2.empty() ? &none : w_ell->data()) : nullptr, (int64_t)chi2.size(), n_samples, M, n_blocks, chi2_max,
                                              out.data());
        if (rc != GPCA_OK) throw Error(rc, std::string("gpca_ldsc_fit: ") + gpca_status_string(rc));
        return out;
    }
    // PC-Relate (gpca_pcrelate): rows [row0, row1) of the lower triangle WITH the diagonal of the ancestry-adjusted kinship, packed as
    // grm packs it; V [N][P] sample coordinates, train (may be null: everyone) [N]; nsnp (may be null) receives the SNPs valid in both
    std::vector<double> pcrelate(const std::vector<double>& V, int32_t P, const std::vector<uint8_t>* train, double tau, int64_t row0,
                                 int64_t row1, std::vector<int32_t>* nsnp = nullptr) const {
        const size_t e = row1 > row0 ? (size_t)(row1 * (row1 + 1) / 2 - row0 * (row0 + 1) / 2) : 0;
        std::vector<double> k(std::max<size_t>(e, 1));
        if (nsnp) nsnp->assign(std::max<size_t>(e, 1), 0);
        check(gpca_pcrelate(h_, V.data(), P, train ? train->data() : nullptr, tau, row0, row1, k.data(), nsnp ? nsnp->data() : nullptr));
        k.resize(e);
        if (nsnp) nsnp->resize(e);
        return k;
    }
    // the regression behind it (gpca_pcrelate_isaf) for kept rows [row0, row1): mu [rows][N] and / or beta [rows][P + 1], not both null
    void pcrelate_isaf(const std::vector<double>& V, int32_t P, const std::vector<uint8_t>* train, int64_t row0, int64_t row1, int64_t n_samples,
                       std::vector<float>* mu, std::vector<float>* beta = nullptr) const {
        const size_t rows = row1 > row0 ? (size_t)(row1 - row0) : 0;
        if (mu) mu->assign(std::max<size_t>(rows * (size_t)n_samples, 1), 0.0f);
        if (beta) beta->assign(std::max<size_t>(rows * (size_t)(P + 1), 1), 0.0f);
        check(gpca_pcrelate_isaf(h_, V.data(), P, train ? train->data() : nullptr, row0, row1, mu ? mu->data() : nullptr, beta ? beta->data() : nullptr));
        if (mu) mu->resize(rows * (size_t)n_samples);
        if (beta) beta->resize(rows * (size_t)(P + 1));
    }

    // linear association scan (gpca_assoc_linear) of kept rows [row0, row1): Y [N][T], C [N][Pc] (may be empty when Pc = 0), include
    // (may be null: everyone) [N]; stats [rows][T][3] = beta, se, t; rowinfo [rows][4] = n_obs, a1_freq, xx, sxx; xb (may be null)
    // [rows][T + Pc]
    void assoc_linear(const std::vector<double>& Y, int32_t T, const std::vector<double>& C, int32_t Pc, const std::vector<uint8_t>* include,
                      double max_vif, int64_t row0, int64_t row1, std::vector<double>& stats, std::vector<double>& rowinfo,
                      std::vector<double>* xb = nullptr) const {
        const size_t rows = row1 > row0 ? (size_t)(row1 - row0) : 0;
        stats.assign(std::max<size_t>(rows * (size_t)T * 3, 1), 0.0);
        rowinfo.assign(std::max<size_t>(rows * 4, 1), 0.0);
        if (xb) xb->assign(std::max<size_t>(rows * (size_t)(T + Pc), 1), 0.0);
        check(gpca_assoc_linear(h_, Y.data(), T, Pc ? C.data() : nullptr, Pc, include ? include->data() : nullptr, max_vif, row0, row1,
                                stats.data(), xb ? xb->data() : nullptr, rowinfo.data()));
        stats.resize(rows * (size_t)T * 3);
        rowinfo.resize(rows * 4);
        if (xb) xb->resize(rows * (size_t)(T + Pc));
    }

    // many-trait QTL scan (gpca_assoc_qtl) of kept rows [row0, row1): Y [N][T], T up to 2^20, C [N][Pc] (may be empty when Pc = 0), include
    // (may be null: everyone) [N]; the pairs of a live row with r2 >= r2_min.  cap = the record buffer; when n_found > cap the records are
    // empty and the caller comes back with cap = n_found.  best = false leaves best_r2 / best_row empty.
    struct QtlResult {
        std::vector<double> rowinfo, yy, xb, r2, best_r2;     // rowinfo [rows][4] = n_obs, a1_freq, xx, sxx; yy [T]; xb, r2 [n_found]
        std::vector<uint32_t> hit_count, rows, traits;        // hit_count [rows]; rows (absolute kept row), traits [n_found]
        std::vector<int64_t> best_row;                        // [T], -1 = no live row
        int64_t n_found = 0;
    };
    QtlResult assoc_qtl(const std::vector<double>& Y, int64_t T, const std::vector<double>& C, int32_t Pc, const std::vector<uint8_t>* include,
                        double max_vif, double r2_min, int64_t cap, int64_t row0, int64_t row1, bool best = true) const {
        const size_t rows = row1 > row0 ? (size_t)(row1 - row0) : 0, nt = T > 0 ? (size_t)T : 0, nc = cap > 0 ? (size_t)cap : 0;
        QtlResult q;
        q.rowinfo.assign(std::max<size_t>(rows * 4, 1), 0.0);
        q.yy.assign(std::max<size_t>(nt, 1), 0.0);
        q.hit_count.assign(std::max<size_t>(rows, 1), 0u);
        std::vector<uint32_t> hi(std::max<size_t>(2 * nc, 1), 0u);
        std::vector<double> hv(std::max<size_t>(2 * nc, 1), 0.0);
        if (best) { q.best_r2.assign(std::max<size_t>(nt, 1), 0.0); q.best_row.assign(std::max<size_t>(nt, 1), -1); }
        check(gpca_assoc_qtl(h_, Y.data(), T, Pc ? C.data() : nullptr, Pc, include ? include->data() : nullptr, max_vif, r2_min, row0, row1,
                             q.rowinfo.data(), q.yy.data(), q.hit_count.data(), cap > 0 ? hi.data() : nullptr, cap > 0 ? hv.data() : nullptr, cap,
                             &q.n_found, best ? q.best_r2.data() : nullptr, best ? q.best_row.data() : nullptr));
        q.rowinfo.resize(rows * 4); q.yy.resize(nt); q.hit_count.resize(rows);
        if (best) { q.best_r2.resize(nt); q.best_row.resize(nt); }
        if (q.n_found <= cap)
            for (int64_t i = 0; i < q.n_found; ++i) {
                q.rows.push_back(hi[2 * (size_t)i]); q.traits.push_back(hi[2 * (size_t)i + 1]);
                q.xb.push_back(hv[2 * (size_t)i]); q.r2.push_back(hv[2 * (size_t)i + 1]);
            }
        return q;
    }

    // logistic score scan (gpca_assoc_logistic_score) of kept rows [row0, row1): Y [N][T] in {0, 1}, C [N][Pc] (may be empty when
    // Pc = 0), include (may be null: everyone) [N], T (Pc + 3) <= 64; stats [rows][T][5] = beta, se, z, vw, V; rowinfo [rows][5] = n_obs,
    // a1_freq, xx, flipped, 0; ua (may be null) [rows][T][Pc + 3] = U, gwg, a_0 .. a_Pc
    void assoc_logistic_score(const std::vector<double>& Y, int32_t T, const std::vector<double>& C, int32_t Pc,
                              const std::vector<uint8_t>* include, double max_vif, int64_t row0, int64_t row1, std::vector<double>& stats,
                              std::vector<double>& rowinfo, std::vector<double>* ua = nullptr) const {
        const size_t rows = row1 > row0 ? (size_t)(row1 - row0) : 0;
        stats.assign(std::max<size_t>(rows * (size_t)T * 5, 1), 0.0);
        rowinfo.assign(std::max<size_t>(rows * 5, 1), 0.0);
        if (ua) ua->assign(std::max<size_t>(rows * (size_t)T * (size_t)(Pc + 3), 1), 0.0);
        check(gpca_assoc_logistic_score(h_, Y.data(), T, Pc ? C.data() : nullptr, Pc, include ? include->data() : nullptr, max_vif, row0, row1,
                                        stats.data(), ua ? ua->data() : nullptr, rowinfo.data()));
        stats.resize(rows * (size_t)T * 5);
        rowinfo.resize(rows * 5);
        if (ua) ua->resize(rows * (size_t)T * (size_t)(Pc + 3));
    }
    // the same scan with the saddle-point correction (gpca_assoc_logistic_spa; gpca.h section a14) of the items with |z| >= spa_z (at
    // least 0.5, or inf): spa [rows][T][4] = -log10 p, status (0 not applied, 1 applied, 2 not converged: the normal value), zeta+, zeta-
    void assoc_logistic_spa(const std::vector<double>& Y, int32_t T, const std::vector<double>& C, int32_t Pc, const std::vector<uint8_t>* include,
                            double max_vif, double spa_z, int64_t row0, int64_t row1, std::vector<double>& stats, std::vector<double>& spa,
                            std::vector<double>& rowinfo, std::vector<double>* ua = nullptr) const {
        const size_t rows = row1 > row0 ? (size_t)(row1 - row0) : 0;
        stats.assign(std::max<size_t>(rows * (size_t)T * 5, 1), 0.0);
        spa.assign(std::max<size_t>(rows * (size_t)T * 4, 1), 0.0);
        rowinfo.assign(std::max<size_t>(rows * 5, 1), 0.0);
        if (ua) ua->assign(std::max<size_t>(rows * (size_t)T * (size_t)(Pc + 3), 1), 0.0);
        check(gpca_assoc_logistic_spa(h_, Y.data(), T, Pc ? C.data() : nullptr, Pc, include ? include->data() : nullptr, max_vif, spa_z, row0, row1,
                                      stats.data(), spa.data(), ua ? ua->data() : nullptr, rowinfo.data()));
        stats.resize(rows * (size_t)T * 5);
        spa.resize(rows * (size_t)T * 4);
        rowinfo.resize(rows * 5);
        if (ua) ua->resize(rows * (size_t)T * (size_t)(Pc + 3));
    }
    // the saddle-point correction for one given vector (gpca_spa_log10p; host only): returns -log10 p; zeta [2] and status may be null
    static double spa_log10p(const std::vector<double>& gt, const std::vector<double>& mu, double u, double* zeta = nullptr, int32_t* status = nullptr) {
        double lp = 0.0;
        const int rc = gt.size() != mu.size() ? GPCA_ERR_BAD_ARG : gpca_spa_log10p(gt.data(), mu.data(), (int64_t)gt.size(), u, &lp, zeta, status);
        if (rc != GPCA_OK) throw Error(rc, std::string("gpca_spa_log10p: ") + gpca_status_string(rc));
        return lp;
    }
    // the same scan with the approximate Firth correction (gpca_assoc_logistic_firth; gpca.h section a15) of the items with |z| >= firth_z
    // (at least 0, or inf): firth [rows][T][5] = -log10 p, status (0 not applied, 1 applied, 2 failed: the normal value), beta (A1), se, D
    void assoc_logistic_firth(const std::vector<double>& Y, int32_t T, const std::vector<double>& C, int32_t Pc, const std::vector<uint8_t>* include,
                              double max_vif, double firth_z, int64_t row0, int64_t row1, std::vector<double>& stats, std::vector<double>& firth,
                              std::vector<double>& rowinfo, std::vector<double>* ua = nullptr) const {
        const size_t rows = row1 > row0 ? (size_t)(row1 - row0) : 0;
        stats.assign(std::max<size_t>(rows * (size_t)T * 5, 1), 0.0);
        firth.assign(std::max<size_t>(rows * (size_t)T * 5, 1), 0.0);
        rowinfo.assign(std::max<size_t>(rows * 5, 1), 0.0);
        if (ua) ua->assign(std::max<size_t>(rows * (size_t)T * (size_t)(Pc + 3), 1), 0.0);
        check(gpca_assoc_logistic_firth(h_, Y.data(), T, Pc ? C.data() : nullptr, Pc, include ? include->data() : nullptr, max_vif, firth_z, row0,
                                        row1, stats.data(), firth.data(), ua ? ua->data() : nullptr, rowinfo.data()));
        stats.resize(rows * (size_t)T * 5);
        firth.resize(rows * (size_t)T * 5);
        rowinfo.resize(rows * 5);
        if (ua) ua->resize(rows * (size_t)T * (size_t)(Pc + 3));
    }
    // the Firth correction for one given vector (gpca_firth_log10p; host only): out [5] = -log10 p, status, beta, se, D
    static void firth_log10p(const std::vector<double>& gt, const std::vector<double>& mu, double u, double* out) {
        const int rc = gt.size() != mu.size() ? GPCA_ERR_BAD_ARG : gpca_firth_log10p(gt.data(), mu.data(), (int64_t)gt.size(), u, out);
        if (rc != GPCA_OK) throw Error(rc, std::string("gpca_firth_log10p: ") + gpca_status_string(rc));
    }
    // the gene-level set scan (gpca_assoc_logistic_set; gpca.h section a16): set_off [n_sets + 1] cuts set_rows into sets of 1 .. 128
    // strictly ascending kept rows; stats / rowinfo / ua per LISTED row as in assoc_logistic_score; phi = set after set, trait after
    // trait, the packed lower triangle of the covariance of the set's scores (allele A1's coding)
    void assoc_logistic_set(const std::vector<double>& Y, int32_t T, const std::vector<double>& C, int32_t Pc, const std::vector<uint8_t>* include,
                            double max_vif, const std::vector<int64_t>& set_off, const std::vector<int64_t>& set_rows, std::vector<double>& stats,
                            std::vector<double>& rowinfo, std::vector<double>& phi, std::vector<double>* ua = nullptr) const {
        if (set_off.size() < 2 || (size_t)set_off.back() != set_rows.size()) throw Error(GPCA_ERR_BAD_ARG, "assoc_logistic_set: set_off does not cut set_rows");
        const size_t rows = set_rows.size();
        size_t tri = 0;
        for (size_t s = 0; s + 1 < set_off.size(); ++s) {
            const size_t m = set_off[s + 1] > set_off[s] ? (size_t)(set_off[s + 1] - set_off[s]) : 0;
            tri += m * (m + 1) / 2;
        }
        stats.assign(std::max<size_t>(rows * (size_t)T * 5, 1), 0.0);
        rowinfo.assign(std::max<size_t>(rows * 5, 1), 0.0);
        phi.assign(std::max<size_t>(tri * (size_t)T, 1), 0.0);
        if (ua) ua->assign(std::max<size_t>(rows * (size_t)T * (size_t)(Pc + 3), 1), 0.0);
        check(gpca_assoc_logistic_set(h_, Y.data(), T, Pc ? C.data() : nullptr, Pc, include ? include->data() : nullptr, max_vif,
                                      (int32_t)(set_off.size() - 1), set_off.data(), set_rows.data(), stats.data(), ua ? ua->data() : nullptr,
                                      rowinfo.data(), phi.data()));
        stats.resize(rows * (size_t)T * 5);
        rowinfo.resize(rows * 5);
        phi.resize(tri * (size_t)T);
        if (ua) ua->resize(rows * (size_t)T * (size_t)(Pc + 3));
    }
    // the burden and SKAT tests of one set (gpca_set_test; host only): out [10] = m_used, burden beta, se, z, -log10 p, SKAT Q, -log10 p,
    // status, z_Q, zeta; weight empty = 1
    static void set_test(const std::vector<double>& u, const std::vector<double>& phi_lower, const std::vector<double>& weight, double* out) {
        const size_t m = u.size();
        const int rc = phi_lower.size() != m * (m + 1) / 2 || (!weight.empty() && weight.size() != m)
                           ? GPCA_ERR_BAD_ARG
                           : gpca_set_test(u.data(), phi_lower.data(), weight.empty() ? nullptr : weight.data(), (int32_t)m, out);
        if (rc != GPCA_OK) throw Error(rc, std::string("gpca_set_test: ") + gpca_status_string(rc));
    }
    // genotype counts inside sample groups (gpca_group_counts; gpca.h section a17): group [N] = 0 .. P - 1 or -1; counts [rows][P][3] =
    // n_obs, n_het, n_hom2 of the kept rows [row0, row1)
    void group_counts(const std::vector<int32_t>& group, int32_t P, int64_t row0, int64_t row1, std::vector<uint32_t>& counts) const {
        const size_t rows = row1 > row0 ? (size_t)(row1 - row0) : 0, p = P > 0 && P <= GPCA_GROUPS_MAX ? (size_t)P : 1;
        counts.assign(std::max<size_t>(rows * p * 3, 1), 0u);
        check(gpca_group_counts(h_, group.data(), P, row0, row1, counts.data()));
        counts.resize(rows * p * 3);
    }
    // f2 jackknife blocks (gpca_f2_blocks; gpca.h section a23): group and the kept rows [row0, row1) as in group_counts, block [rows] =
    // the block 0 .. B - 1 of every row of the band or -1; acc and cnt [B][P (P - 1) / 2] are WRITTEN (the caller adds its bands);
    // counts, when asked for, = group_counts' [rows][P][3] of the band from the same genotype pass
    void f2_blocks(const std::vector<int32_t>& group, int32_t P, int64_t row0, int64_t row1, const std::vector<int32_t>& block, int32_t B,
                   std::vector<int64_t>& acc, std::vector<int64_t>& cnt, std::vector<uint32_t>* counts = nullptr) const {
        const size_t rows = row1 > row0 ? (size_t)(row1 - row0) : 0, p = P > 1 && P <= GPCA_GROUPS_MAX ? (size_t)P : 2;
        const size_t nout = (size_t)std::max<int32_t>(B, 1) * (p * (p - 1) / 2);
        if (block.size() != rows) throw Error(GPCA_ERR_BAD_ARG, "gpca_f2_blocks: one block id per row of the band");
        acc.assign(nout, 0); cnt.assign(nout, 0);
        if (counts) counts->assign(std::max<size_t>(rows * p * 3, 1), 0u);
        const int32_t none = 0;
        check(gpca_f2_blocks(h_, group.data(), P, row0, row1, rows ? block.data() : &none, B, acc.data(), cnt.data(), counts ? counts->data() : nullptr));
        if (counts) counts->resize(rows * p * 3);
    }
    // f2, f3 and f4 with their weighted block-jackknife standard errors (gpca_fstat; host only): acc and cnt [B][pairs] = the bands of
    // f2_blocks added up, quads [M][4] = (a, b, c, d) read as f4(a, b; c, d); returns [M][6] = theta, theta_J, se, z, blocks used, min SNPs
    static std::vector<double> fstat(const std::vector<int64_t>& acc, const std::vector<int64_t>& cnt, int32_t B, int32_t P,
                                     const std::vector<int32_t>& quads) {
        const size_t M = quads.size() / 4, pairs = P > 1 ? (size_t)P * (size_t)(P - 1) / 2 : 0;
        std::vector<double> out(std::max<size_t>(6 * M, 1), 0.0);
        int rc = quads.size() != 4 * M || B < 1 || acc.size() != (size_t)B * pairs || cnt.size() != acc.size() ? GPCA_ERR_BAD_ARG : GPCA_OK;
        const int32_t none[4] = {0, 0, 0, 0};
        if (rc == GPCA_OK) rc = gpca_fstat(acc.data(), cnt.data(), B, P, M ? quads.data() : none, (int64_t)M, out.data());
        if (rc != GPCA_OK) throw Error(rc, std::string("gpca_fstat: ") + gpca_status_string(rc));
        out.resize(6 * M);
        return out;
    }
    // Hudson's Fst of every pair of groups (gpca_fst_hudson; host only): sums [P (P - 1) / 2][3] is ADDED TO (zero it before the first
    // band); num / den [rows][pairs] when asked for
    static void fst_hudson(const std::vector<uint32_t>& counts, int32_t P, std::vector<double>& sums, std::vector<double>* num = nullptr,
                           std::vector<double>* den = nullptr) {
        const size_t per = P > 0 ? (size_t)P * 3 : 1, rows = counts.size() / per, pairs = P > 1 ? (size_t)P * (size_t)(P - 1) / 2 : 0;
        int rc = counts.size() != rows * per || sums.size() != pairs * 3 ? GPCA_ERR_BAD_ARG : GPCA_OK;
        if (rc == GPCA_OK) {
            if (num) num->assign(std::max<size_t>(rows * pairs, 1), 0.0);
            if (den) den->assign(std::max<size_t>(rows * pairs, 1), 0.0);
            rc = gpca_fst_hudson(counts.data(), (int64_t)rows, P, num ? num->data() : nullptr, den ? den->data() : nullptr, sums.data());
            if (num) num->resize(rows * pairs);
            if (den) den->resize(rows * pairs);
        }
        if (rc != GPCA_OK) throw Error(rc, std::string("gpca_fst_hudson: ") + gpca_status_string(rc));
    }
    // Weir and Cockerham's Fst over the groups with use[p] != 0 (empty: all) (gpca_fst_wc; host only): sums [3] is ADDED TO; abc [rows][3]
    // when asked for
    static void fst_wc(const std::vector<uint32_t>& counts, int32_t P, const std::vector<uint8_t>& use, double* sums,
                       std::vector<double>* abc = nullptr) {
        const size_t per = P > 0 ? (size_t)P * 3 : 1, rows = counts.size() / per;
        int rc = counts.size() != rows * per || (!use.empty() && use.size() != (size_t)P) ? GPCA_ERR_BAD_ARG : GPCA_OK;
        if (rc == GPCA_OK) {
            if (abc) abc->assign(std::max<size_t>(rows * 3, 1), 0.0);
            rc = gpca_fst_wc(counts.data(), (int64_t)rows, P, use.empty() ? nullptr : use.data(), abc ? abc->data() : nullptr, sums);
            if (abc) abc->resize(rows * 3);
        }
        if (rc != GPCA_OK) throw Error(rc, std::string("gpca_fst_wc: ") + gpca_status_string(rc));
    }
    // genotype counts per sample (gpca_sample_counts; gpca.h section a18) over the kept rows [row0, row1): counts [N][3] = n_obs, n_het,
    // n_hom2; with q (one weight per row of the band, each <= 2^30) qsum [N] = the sum of q over the rows on which the sample is
    // observed.  WRITTEN per call: the caller sums its bands.
    void sample_counts(int64_t row0, int64_t row1, const std::vector<uint32_t>* q, std::vector<uint32_t>& counts,
                       std::vector<uint64_t>* qsum = nullptr) const {
        const size_t N = (size_t)dims().second, rows = row1 > row0 ? (size_t)(row1 - row0) : 0;
        if ((q != nullptr) != (qsum != nullptr) || (q && q->size() != rows))
            throw std::invalid_argument("sample_counts: q (one entry per row of the band) and qsum go together");
        counts.assign(std::max<size_t>(3 * N, 1), 0u);
        if (qsum) qsum->assign(std::max<size_t>(N, 1), 0u);
        static const uint32_t none = 0;
        check(gpca_sample_counts(h_, row0, row1, q ? (rows ? q->data() : &none) : nullptr, counts.data(), qsum ? qsum->data() : nullptr));
        counts.resize(3 * N);
        if (qsum) qsum->resize(N);
    }
    // runs of homozygosity (gpca_roh; gpca.h section a20) over the kept rows [row0, row1) and all samples: brk = one byte per row of the
    // band (bit 0: a window domain starts, bit 1: no run continues into the row); segs [n][5] = sample, first, last, n_het, n_missing in
    // ascending (sample, first) order, seg_count [N].  Comes back with a larger buffer itself when the first one was short.
    void roh(int64_t row0, int64_t row1, const std::vector<uint8_t>& brk, const gpca_roh_params& params, std::vector<uint32_t>& segs,
             std::vector<uint32_t>& seg_count) const {
        const size_t N = (size_t)dims().second, rows = row1 > row0 ? (size_t)(row1 - row0) : 0;
        if (brk.size() != rows) throw std::invalid_argument("roh: brk needs one entry per row of the band");
        seg_count.assign(std::max<size_t>(N, 1), 0u);
        static const uint8_t none = 0;
        int64_t cap = (int64_t)std::max<size_t>(4 * N, 1024), found = 0;
        for (;;) {
            segs.assign((size_t)cap * 5, 0u);
            check(gpca_roh(h_, row0, row1, rows ? brk.data() : &none, &params, seg_count.data(), segs.data(), cap, &found));
            if (found <= cap) break;
            cap = found;
        }
        segs.resize((size_t)found * 5);
        seg_count.resize(N);
    }
    // admixture proportions (gpca.h section a21) over the kept rows and all samples: Q [N][K], F [Kr][K] (Kr = num_pca_snps()); mode [N]
    // (0 = free, 1 = Q fixed, 2 = projected) or NULL.  admix_init: the starting point of a seed; admix_step: one EM step from Q and F as
    // given, returns the log-likelihood of (Q, F); admix: the fit, from the seed's init (params.init = 0) or from Q and F (1); trace
    // receives the cycle-start log-likelihoods (the first 2^20 at most).
    void admix_init(int32_t K, uint64_t seed, std::vector<float>& Q, std::vector<float>& F) const {
        const size_t N = (size_t)dims().second, Kr = (size_t)gpca_num_pca_snps(h_), k = (size_t)std::max<int32_t>(K, 1);
        Q.assign(std::max<size_t>(N * k, 1), 0.0f); F.assign(std::max<size_t>(Kr * k, 1), 0.0f);
        check(gpca_admix_init(h_, K, seed, Q.data(), F.data()));
        Q.resize(N * k); F.resize(Kr * k);
    }
    double admix_step(int32_t K, const std::vector<float>& Q, const std::vector<float>& F, const std::vector<uint8_t>* mode, std::vector<float>& Qn,
                      std::vector<float>& Fn) const {
        const size_t N = (size_t)dims().second, Kr = (size_t)gpca_num_pca_snps(h_), k = (size_t)std::max<int32_t>(K, 1);
        if (Q.size() != N * k || F.size() != Kr * k || (mode && mode->size() != N)) throw std::invalid_argument("admix_step: Q [N][K], F [Kr][K], mode [N]");
        Qn.assign(std::max<size_t>(Q.size(), 1), 0.0f); Fn.assign(std::max<size_t>(F.size(), 1), 0.0f);
        double ll = 0.0;
        check(gpca_admix_step(h_, K, Q.data(), F.data(), mode ? mode->data() : nullptr, Qn.data(), Fn.data(), &ll));
        Qn.resize(Q.size()); Fn.resize(F.size());
        return ll;
    }
    gpca_admix_info admix(const gpca_admix_params& params, const std::vector<uint8_t>* mode, std::vector<float>& Q, std::vector<float>& F,
                          std::vector<double>* trace = nullptr) const {
        const size_t N = (size_t)dims().second, Kr = (size_t)gpca_num_pca_snps(h_), k = (size_t)std::max<int32_t>(params.K, 1);
        if (mode && mode->size() != N) throw std::invalid_argument("admix: mode needs one byte per sample");
        if (params.init == 1 && (Q.size() != N * k || F.size() != Kr * k)) throw std::invalid_argument("admix: init = 1 needs Q [N][K] and F [Kr][K]");
        if (params.init != 1) { Q.assign(std::max<size_t>(N * k, 1), 0.0f); F.assign(std::max<size_t>(Kr * k, 1), 0.0f); }
        std::vector<double> tr((size_t)std::min<int32_t>(std::max<int32_t>(params.max_iter, 1), 1 << 20), 0.0);   // (a cycle is at least one step)
        gpca_admix_info info{};
        info.trace = tr.data(); info.trace_cap = (int64_t)tr.size();
        check(gpca_admix(h_, &params, mode ? mode->data() : nullptr, Q.data(), F.data(), &info));
        Q.resize(N * k); F.resize(Kr * k);
        if (trace) trace->assign(tr.begin(), tr.begin() + (size_t)std::min<int64_t>(info.cycles, info.trace_cap));
        info.trace = nullptr; info.trace_cap = 0;
        return info;
    }
    // one hold-out step (gpca.h section a22): admix_step with the observed calls of fold `fold` of `folds` under cv_seed counted as
    // missing; held = held_loglik, n_held, n_het_held of those calls at (Q, F).  Returns the training log-likelihood.
    struct AdmixHeld { double held_loglik; int64_t n_held, n_het_held; };
    double admix_step_holdout(int32_t K, const std::vector<float>& Q, const std::vector<float>& F, const std::vector<uint8_t>* mode, int32_t folds,
                              int32_t fold, uint64_t cv_seed, std::vector<float>& Qn, std::vector<float>& Fn, AdmixHeld& held) const {
        const size_t N = (size_t)dims().second, Kr = (size_t)gpca_num_pca_snps(h_), k = (size_t)std::max<int32_t>(K, 1);
        if (Q.size() != N * k || F.size() != Kr * k || (mode && mode->size() != N)) throw std::invalid_argument("admix_step_holdout: Q [N][K], F [Kr][K], mode [N]");
        Qn.assign(std::max<size_t>(Q.size(), 1), 0.0f); Fn.assign(std::max<size_t>(F.size(), 1), 0.0f);
        double ll = 0.0;
        check(gpca_admix_step_holdout(h_, K, Q.data(), F.data(), mode ? mode->data() : nullptr, folds, fold, cv_seed, Qn.data(), Fn.data(), &ll,
                                      &held.held_loglik, &held.n_held, &held.n_het_held));
        Qn.resize(Q.size()); Fn.resize(F.size());
        return ll;
    }
    // the cross-validation error of the fit (gpca.h section a22): per fold the fit with the fold's observed calls hidden, then their
    // deviance; from the seed's init (params.init = 0) or from Q0 and F0 (1).  Returns cv_error; folds_out [folds].
    double admix_cv(const gpca_admix_params& params, const std::vector<uint8_t>* mode, int32_t folds, uint64_t cv_seed, const std::vector<float>* Q0,
                    const std::vector<float>* F0, std::vector<gpca_admix_cv_fold_info>& folds_out) const {
        const size_t N = (size_t)dims().second, Kr = (size_t)gpca_num_pca_snps(h_), k = (size_t)std::max<int32_t>(params.K, 1);
        if (mode && mode->size() != N) throw std::invalid_argument("admix_cv: mode needs one byte per sample");
        if (params.init == 1 && (!Q0 || !F0 || Q0->size() != N * k || F0->size() != Kr * k)) throw std::invalid_argument("admix_cv: init = 1 needs Q0 [N][K] and F0 [Kr][K]");
        folds_out.assign((size_t)std::min<int32_t>(std::max<int32_t>(folds, 1), GPCA_ADMIX_CV_MAX_FOLDS), gpca_admix_cv_fold_info{});
        double cv = 0.0;
        check(gpca_admix_cv(h_, &params, mode ? mode->data() : nullptr, folds, cv_seed, params.init == 1 ? Q0->data() : nullptr,
                            params.init == 1 ? F0->data() : nullptr, folds_out.data(), &cv));
        return cv;
    }
    // the host rule on the records (gpca_roh_select; host only): keep [n] by length in bp and bp per SNP; pos [K] = the kept rows' positions
    static std::vector<uint8_t> roh_select(const std::vector<uint32_t>& segs, const std::vector<int64_t>& pos, int64_t min_bp, int64_t max_bp_per_snp) {
        const size_t n = segs.size() / 5;
        std::vector<uint8_t> keep(std::max<size_t>(n, 1), 0);
        int rc = segs.size() != 5 * n ? GPCA_ERR_BAD_ARG : GPCA_OK;
        for (size_t i = 0; rc == GPCA_OK && i < n; ++i)
            if (segs[5 * i + 1] >= pos.size() || segs[5 * i + 2] >= pos.size()) rc = GPCA_ERR_BAD_ARG;
        if (rc == GPCA_OK && n) rc = gpca_roh_select(segs.data(), (int64_t)n, pos.data(), min_bp, max_bp_per_snp, keep.data());
        if (rc != GPCA_OK) throw Error(rc, std::string("gpca_roh_select: ") + gpca_status_string(rc));
        keep.resize(n);
        return keep;
    }
    // the rows' weights for the heterozygosity F (gpca_het_weights; host only): qc [rows][4] as snp_qc_detail gives them
    static std::vector<uint32_t> het_weights(const std::vector<uint32_t>& qc) {
        const size_t rows = qc.size() / 4;
        std::vector<uint32_t> q(std::max<size_t>(rows, 1), 0u);
        const int rc = qc.size() != rows * 4 ? GPCA_ERR_BAD_ARG : (rows ? gpca_het_weights(qc.data(), (int64_t)rows, q.data()) : GPCA_OK);
        if (rc != GPCA_OK) throw Error(rc, std::string("gpca_het_weights: ") + gpca_status_string(rc));
        q.resize(rows);
        return q;
    }
    // O_HOM, E_HOM and F of every sample (gpca_sample_het; host only): out [N][3]
    static std::vector<double> sample_het(const std::vector<uint32_t>& counts, const std::vector<uint64_t>& qsum) {
        const size_t N = qsum.size();
        std::vector<double> out(std::max<size_t>(3 * N, 1), 0.0);
        const int rc = counts.size() != 3 * N ? GPCA_ERR_BAD_ARG : (N ? gpca_sample_het(counts.data(), qsum.data(), (int64_t)N, out.data()) : GPCA_OK);
        if (rc != GPCA_OK) throw Error(rc, std::string("gpca_sample_het: ") + gpca_status_string(rc));
        out.resize(3 * N);
        return out;
    }
    // the null logistic model of one trait (gpca_logistic_null; host only): y [N] in {0, 1}, C [N][Pc]; alpha [Pc + 1], mu [N] (0 outside
    // the included samples); returns the number of Newton steps; throws Error with the status (no message: there is no handle)
    static int logistic_null(const std::vector<double>& y, const std::vector<double>& C, int32_t Pc, const std::vector<uint8_t>* include,
                             std::vector<double>& alpha, std::vector<double>& mu) {
        alpha.assign((size_t)Pc + 1, 0.0);
        mu.assign(std::max<size_t>(y.size(), 1), 0.0);
        int32_t iters = 0;
        const int rc = gpca_logistic_null(y.data(), Pc ? C.data() : nullptr, Pc, include ? include->data() : nullptr, (int64_t)y.size(), alpha.data(),
                                          mu.data(), &iters);
        if (rc != GPCA_OK) throw Error(rc, std::string("gpca_logistic_null: ") + gpca_status_string(rc));
        mu.resize(y.size());
        return (int)iters;
    }
    static double normal_log10p(double z) { return gpca_normal_log10p(z); }

private:
    gpca_handle* h_ = nullptr;
    int k_ = 0;
    int device_ = -1, precision_ = GPCA_PREC_I8_EXACT, storage_ = GPCA_STORE_INT8, digit_planes_ = 0;
};

struct LdBlockSpecification {                       // prepare.rs:1540-1543
    std::string user_defined_block_tag;
    std::vector<PcaSnpId> pca_snp_ids_in_block;
};

/* impl PcaReadyGenotypeAccessor for MicroarrayGenotypeAccessor (prepare.rs:1838-2030), backed by genotypes resident in
 * HBM (or streamed panels) instead of the IoService actor pool.  Copyable like the reference's `Clone` accessor: copies
 * share the engine: pulls from different threads run concurrently on the handle's lanes, every other call waits for them (gpca.h,
 * "Threading"). */
class MicroarrayGenotypeAccessor {
public:
    explicit MicroarrayGenotypeAccessor(Engine& e) : eng_(&e) {}
    std::vector<float> get_standardized_snp_sample_block(const std::vector<PcaSnpId>& pca_snp_ids_to_fetch,
                                                         const std::vector<QcSampleId>& qc_sample_ids_to_fetch) const {
        return eng_->standardize_block(pca_snp_ids_to_fetch, qc_sample_ids_to_fetch);
    }
    int64_t num_pca_snps() const { return eng_->num_pca_snps(); }
    int64_t num_qc_samples() const { return eng_->num_qc_samples(); }
    std::vector<int64_t> original_indices_of_pca_snps() const { return eng_->pca_snp_rows(); }
    Engine& engine() const { return *eng_; }
private:
    Engine* eng_;
};

struct EigenSNPCoreAlgorithmConfig {                // main.rs:311-327 with clap's effective defaults (main.rs:561-588)
    int target_num_global_pcs = 10;
    int components_per_ld_block = 7;
    double subset_factor_for_local_basis_learning = 0.075;
    int64_t min_subset_size_for_local_basis_learning = 10000;
    int64_t max_subset_size_for_local_basis_learning = 40000;
    int global_pca_sketch_oversampling = 10;
    int global_pca_num_power_iterations = 2;
    int local_rsvd_sketch_oversampling = 10;
    int local_rsvd_num_power_iterations = 2;
    uint64_t random_seed = 2025;
    int64_t snp_processing_strip_size = 2000;
    int refine_pass_count = 1;
    bool collect_diagnostics = false;
    int64_t diagnostic_block_list_id_to_trace = -1;
};

struct EigenSNPCoreOutput {
    std::vector<float> final_sample_principal_component_scores;    // [N][K]  main.rs:389
    std::vector<double> final_principal_component_eigenvalues;     // [K]     main.rs:394
    std::vector<float> final_snp_principal_component_loadings;     // [D][K]  main.rs:407
    int64_t num_qc_samples_used = 0, num_pca_snps_used = 0;
    int num_principal_components_computed = 0;
    // compute_pca(..., project_all = true): every sample projected onto the fit (gpca_transform, [N][K]), taken while the fit is valid --
    // before the keep mask of the blocks' union is restored (which drops the fit)
    std::vector<double> projected_sample_scores;
};

/* EigenSNPCoreAlgorithm::new(cfg).compute_pca(&accessor, &blocks) (main.rs:359-365): top-K PCA of the standardised matrix
 * restricted to the SNPs the blocks name (a PCA SNP in no block leaves the PCA, prepare.rs:1465-1469).
 *   local_stage = false (default): ONE global randomized PCA over the union of the blocks (target_num_global_pcs,
 *     global_pca_sketch_oversampling, global_pca_num_power_iterations, random_seed act).
 *   local_stage = true: the multi-stage algorithm the 14 config fields parameterise, as published for the un-vendored
 *     efficient_pca crate (parity UNPINNED): sample subset -> per-block local bases -> condensed features of all samples, row
 *     standardised -> initial global randomized PCA of the condensed features -> refine_pass_count refinement passes on the full
 *     matrix.  Same stages, same calls, same seeds as genomic_pca_amd.engine.EigenSNPCoreAlgorithm._multi_stage. */
class EigenSNPCoreAlgorithm {
public:
    explicit EigenSNPCoreAlgorithm(const EigenSNPCoreAlgorithmConfig& cfg) : cfg_(cfg) {}

    static int64_t subset_size(const EigenSNPCoreAlgorithmConfig& cfg, int64_t n_samples) {
        int64_t want = (int64_t)std::nearbyint(cfg.subset_factor_for_local_basis_learning * (double)n_samples);
        want = std::max(cfg.min_subset_size_for_local_basis_learning, std::min(cfg.max_subset_size_for_local_basis_learning, want));
        return std::max<int64_t>(2, std::min(n_samples, want));
    }
    /* the first ns entries of a Fisher-Yates shuffle driven by SplitMix64(seed); empty = every sample */
    static std::vector<uint8_t> subset_mask(const EigenSNPCoreAlgorithmConfig& cfg, int64_t n_samples) {
        const int64_t ns = subset_size(cfg, n_samples);
        if (ns >= n_samples) return {};
        std::vector<int64_t> idx((size_t)n_samples);
        for (int64_t i = 0; i < n_samples; ++i) idx[(size_t)i] = i;
        uint64_t state = cfg.random_seed;
        for (int64_t i = 0; i < ns; ++i) {
            state += 0x9E3779B97F4A7C15ull;
            uint64_t z = state;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            z ^= z >> 31;
            const int64_t j = i + (int64_t)(z % (uint64_t)(n_samples - i));
            std::swap(idx[(size_t)i], idx[(size_t)j]);
        }
        std::vector<uint8_t> mask((size_t)n_samples, 0);
        for (int64_t i = 0; i < ns; ++i) mask[(size_t)idx[(size_t)i]] = 1;
        return mask;
    }

    EigenSNPCoreOutput compute_pca(const MicroarrayGenotypeAccessor& accessor, const std::vector<LdBlockSpecification>& ld_blocks,
                                   bool local_stage = false, bool project_all = false) const {
        Engine& eng = accessor.engine();
        const int64_t n_pca = accessor.num_pca_snps();
        if (ld_blocks.empty()) throw std::invalid_argument("compute_pca: ld_block_specifications is empty");
        std::vector<PcaSnpId> ids;
        for (const auto& b : ld_blocks) ids.insert(ids.end(), b.pca_snp_ids_in_block.begin(), b.pca_snp_ids_in_block.end());
        std::sort(ids.begin(), ids.end());
        ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
        if (ids.empty()) throw std::invalid_argument("compute_pca: the LD blocks hold no PCA SNP");
        if (ids.front() < 0 || ids.back() >= n_pca)
            throw std::invalid_argument("compute_pca: PcaSnpId " + std::to_string(ids.front() < 0 ? ids.front() : ids.back()) + " out of range [0, " +
                                        std::to_string(n_pca) + ")");
        SnpStats saved;
        std::vector<int64_t> rows;
        const bool restrict_rows = (int64_t)ids.size() < n_pca;
        if (restrict_rows || local_stage) { saved = eng.get_standardization(); rows = eng.pca_snp_rows(); }
        if (restrict_rows) {   // keep mask = union of the blocks (same mu / sigma); the accessor's numbering is restored afterwards
            std::vector<uint8_t> keep2(saved.keep.size(), 0);
            for (PcaSnpId id : ids) keep2[(size_t)rows[(size_t)id]] = 1;
            eng.set_standardization(saved.mu, saved.sigma, keep2);
        }
        EigenSNPCoreOutput out;
        try {
            if (local_stage) multi_stage(eng, ld_blocks, saved, rows);
            else eng.rsvd(cfg_.target_num_global_pcs, cfg_.global_pca_sketch_oversampling, cfg_.global_pca_num_power_iterations, cfg_.random_seed);
            out.final_sample_principal_component_scores = eng.scores();
            out.final_principal_component_eigenvalues = eng.eigenvalues();
            out.final_snp_principal_component_loadings = eng.loadings();
            out.num_qc_samples_used = accessor.num_qc_samples();
            out.num_pca_snps_used = (int64_t)ids.size();
            out.num_principal_components_computed = eng.components();   // (the local stage may leave fewer: min(K, condensed features))
            if (project_all) out.projected_sample_scores = eng.transform();
        } catch (...) {
            if (restrict_rows) eng.set_standardization(saved.mu, saved.sigma, saved.keep);
            throw;
        }
        if (restrict_rows) eng.set_standardization(saved.mu, saved.sigma, saved.keep);
        return out;
    }

private:
    void multi_stage(Engine& eng, const std::vector<LdBlockSpecification>& ld_blocks, const SnpStats& st, const std::vector<int64_t>& pca_rows) const {
        const auto dm = eng.dims();
        const int64_t M = dm.first, N = dm.second;
        const int K = cfg_.target_num_global_pcs;
        const std::vector<uint8_t> mask = subset_mask(cfg_, N);
        int64_t n_sub = N;
        if (!mask.empty()) { n_sub = 0; for (uint8_t m : mask) n_sub += m; }
        std::vector<std::vector<int64_t>> blocks;
        int64_t longest = 0;
        for (const auto& b : ld_blocks) {
            if (b.pca_snp_ids_in_block.empty()) continue;
            std::vector<int64_t> r;
            for (PcaSnpId id : b.pca_snp_ids_in_block) r.push_back(pca_rows[(size_t)id]);
            std::sort(r.begin(), r.end());
            longest = std::max<int64_t>(longest, (int64_t)r.size());
            blocks.push_back(std::move(r));
        }
        const int64_t cp = std::max(1, cfg_.components_per_ld_block);
        const int cmax = (int)std::min<int64_t>({cp, longest, n_sub});
        std::vector<float> W((size_t)M * (size_t)cmax, 0.f);
        std::vector<int32_t> feat0((size_t)M, -1);
        int64_t R = 0;
        {
            Engine sub(eng.device(), eng.precision(), eng.storage(), eng.digit_planes());
            {   // sized once for the widest block: every block reuses its buffers
                size_t big = 0;
                for (size_t bi = 1; bi < blocks.size(); ++bi)
                    if (blocks[bi].back() - blocks[bi].front() > blocks[big].back() - blocks[big].front()) big = bi;
                sub.copy_rows_from(eng, blocks[big].front(), blocks[big].back() + 1 - blocks[big].front());
            }
            for (size_t bi = 0; bi < blocks.size(); ++bi) {
                const std::vector<int64_t>& rows = blocks[bi];
                const int64_t r0 = rows.front(), r1 = rows.back() + 1, D = (int64_t)rows.size();
                sub.copy_rows_from(eng, r0, r1 - r0);
                std::vector<uint8_t> keep((size_t)(r1 - r0), 0);
                for (int64_t r : rows) keep[(size_t)(r - r0)] = 1;
                sub.set_standardization(std::vector<float>(st.mu.begin() + r0, st.mu.begin() + r1), std::vector<float>(st.sigma.begin() + r0, st.sigma.begin() + r1), keep);
                sub.set_sample_mask(mask.empty() ? nullptr : &mask);
                int c = (int)std::min<int64_t>({cp, D, n_sub});
                const int lo = (int)std::max<int64_t>(0, std::min<int64_t>(cfg_.local_rsvd_sketch_oversampling, std::min(D, n_sub) - c));
                sub.rsvd(c, lo, cfg_.local_rsvd_num_power_iterations, cfg_.random_seed + 1 + (uint64_t)bi);
                const std::vector<float> U = sub.loadings();          // [D][c]
                const std::vector<double> feats = sub.transform();    // [N][c]
                int kept_cols = 0;
                for (int j = 0; j < c; ++j) {
                    double mean = 0.0;
                    for (int64_t n = 0; n < N; ++n) mean += feats[(size_t)n * c + j];
                    mean /= (double)N;
                    double ss = 0.0;
                    for (int64_t n = 0; n < N; ++n) { const double d = feats[(size_t)n * c + j] - mean; ss += d * d; }
                    const double sd = std::sqrt(ss / (double)(N - 1));
                    if (!(sd > 1e-12)) continue;
                    const float sdf = (float)sd;
                    for (int64_t a = 0; a < D; ++a) W[(size_t)rows[(size_t)a] * cmax + kept_cols] = U[(size_t)a * c + j] / sdf;
                    ++kept_cols;
                }
                if (kept_cols == 0) continue;
                for (int64_t r : rows) feat0[(size_t)r] = (int32_t)R;
                R += kept_cols;
            }
        }
        if (R < 1) throw std::invalid_argument("compute_pca: no condensed features (every local component is constant)");
        eng.set_sample_mask(nullptr);
        eng.set_condensed_basis(W, feat0, cmax, R);
        const int k0 = (int)std::min<int64_t>(K, R);
        const int go = (int)std::max<int64_t>(0, std::min<int64_t>(cfg_.global_pca_sketch_oversampling, std::min(R, N) - k0));
        eng.rsvd_condensed(k0, go, cfg_.global_pca_num_power_iterations, cfg_.random_seed);
        std::vector<double> scores = eng.scores_f64();
        for (int pass = 0; pass < std::max(1, cfg_.refine_pass_count); ++pass) { eng.refine(scores, k0); scores = eng.scores_f64(); }
    }

    EigenSNPCoreAlgorithmConfig cfg_;
};

/* PCA::new(), .rfit(x, k, n_oversamples, seed, tol), .transform(x) (main.rs:602, 648-660).  The reference hands rfit an
 * Array2<f64> samples x variants (vcf.rs:329-342) by value; here the same matrix goes in as the int8 dosages it was built
 * from, SNP-major (variants x samples): 1 B per genotype instead of build_matrix's 8 B + clone (main.rs:640). */
class PCA {
public:
    explicit PCA(int device = -1, int precision = GPCA_PREC_I8_EXACT, int storage = GPCA_STORE_INT8) : eng_(device, precision, storage) {}
    PCA& rfit(const int8_t* variants_by_samples, int64_t n_features, int64_t n_samples, int k, int n_oversamples = 10, uint64_t seed = 0,
              int power_iters = 2) {
        if (k == 0) throw std::invalid_argument("Number of components (-k) must be > 0.");                                       // main.rs:607-609
        if (n_samples < 2) throw std::invalid_argument("PCA requires at least 2 samples, found " + std::to_string(n_samples) + ".");  // main.rs:614-616
        if (n_features == 0) throw std::invalid_argument("PCA requires at least 1 variant (feature), found 0.");                 // main.rs:617-619
        k = (int)std::min<int64_t>({(int64_t)k, n_samples, n_features});                                                          // main.rs:621-628
        eng_.upload_genotypes_i8(variants_by_samples, n_features, n_samples, n_samples);
        eng_.snp_stats(QcConfig::none(), false);
        // zero-variance rows leave the PCA even without QC thresholds: the reference's clamp (main.rs:621-628), applied to what is left
        if (eng_.num_pca_snps() == 0) throw std::invalid_argument("PCA requires at least 1 variant (feature), found 0.");
        k = (int)std::min<int64_t>((int64_t)k, eng_.num_pca_snps());
        const int64_t l = std::min<int64_t>({(int64_t)k + n_oversamples, n_samples, eng_.num_pca_snps()});
        eng_.rsvd(k, (int)(l - k), power_iters, seed);
        fitted_ = true;
        return *this;
    }
    std::vector<double> transform() const {       // N x k, f64 like the reference's Array2<f64> (main.rs:659)
        if (!fitted_) throw std::logic_error("PCA.transform before rfit");
        return eng_.transform();
    }
    std::vector<double> explained_variance() const { return eng_.eigenvalues(); }
    std::vector<float> rotation() const { return eng_.loadings(); }
    int components() const { return eng_.components(); }
    Engine& engine() { return eng_; }
private:
    Engine eng_;
    bool fitted_ = false;
};

}  // namespace gpca

#endif /* GPCA_HPP */
