// genomic_pca -- the reference's command line (main.rs:501-593) over the MI355X engine, as a native host program.
//
// Two workflows, dispatched on --eigensnp like main.rs:109-122:
//   * VCF  (run_vcf_workflow, main.rs:133-247):  --vcf-dir D -k K [--maf f] [--rfit-seed s] --out P
//         -> P.vcf.pca.tsv, P.eigenvalues.tsv (header only, as main.rs:676 leaves the vector empty;
//            --write-eigenvalues is an extension that fills it)
//   * BED  (run_eigensnp_rust_workflow, main.rs:250-442):  --eigensnp --bed-file B --ld-block-file L --out P [--eigensnp-*]
//         -> P.eigensnp.pca.tsv, P.eigenvalues.tsv, P.eigensnp.loadings.tsv
// Everything numerical happens behind include/gpca.h (libgpca.so, hand-written HIP); this file parses text, maps the
// .bed, and writes TSVs.  Same flags, defaults, messages and output bytes as `python -m genomic_pca_amd`
// (genomic_pca_amd/cli.py), which tests/test_cpp_host.py holds it to.
#include <dirent.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "formats.hpp"
#include "gpca.hpp"

namespace {

struct Args {
    std::string output_prefix, vcf_dir, bed_file, ld_block_file, sample_keep_file, log_level = "Info";
    bool have_components = false, have_maf = false, have_seed = false, eigensnp = false, collect_diagnostics = false, write_eigenvalues = false;
    int64_t components = 0, threads = 0;
    double maf = 0.01;
    uint64_t rfit_seed = 0;
    // clap's effective defaults when --eigensnp is given (main.rs:545-588)
    double min_call_rate = 0.98, min_maf = 0.01, max_hwe_p = 1e-6, subset_factor = 0.075;
    int64_t k_global = 10, components_per_block = 7, min_subset = 10000, max_subset = 40000, global_oversampling = 10, global_power_iter = 2,
            local_oversampling = 10, local_power_iter = 2, strip_size = 2000, refine_passes = 1, rfit_power_iters = 2;
    uint64_t seed = 2025;
    // extensions
    int device = -1;
    std::string precision = "i8", storage = "auto", stream = "auto";
    int64_t panel_rows = 0;
    bool local_stage = false;
    bool save_model = false;          // --gpca-save-model: also write P.eigensnp.model.tsv
    std::string project_model;        // --gpca-project-model MODEL: project --bed-file's samples onto it
    bool make_grm = false;            // --gpca-make-grm: also write P.grm.bin / P.grm.N.bin / P.grm.id
    std::string grm_scaling = "standardized";
    bool make_king = false;           // --gpca-make-king: also write P.kin0
    bool have_king_filter = false, have_king_cutoff = false;
    double king_filter = 0.0, king_cutoff = 0.0;   // --gpca-king-table-filter X, --gpca-king-cutoff X
    bool make_pcrelate = false;       // --gpca-make-pcrelate P: also write P.pcrelate.kin / P.pcrelate.inbreed, adjusted for the first P PCs
    int64_t pcrelate_pcs = 0;
    bool have_pcrelate_tau = false, have_pcrelate_filter = false;
    double pcrelate_tau = 0.01, pcrelate_filter = 0.0;   // --gpca-pcrelate-maf-bound T, --gpca-pcrelate-table-filter X
    bool have_indep = false;          // --gpca-indep-pairwise WINDOW R2: LD pruning of the kept SNPs before the GRM, KING and the PCA
    std::string indep_window, indep_r2_text;
    double indep_r2 = 0.0;
    std::string ld_score;             // --gpca-ld-score WINDOW: the LD score of every SNP that passes the SNP QC, after the PCA outputs
    bool assoc_ldsc = false;          // --gpca-assoc-ldsc: LD-score regression of every trait's scan statistics on those LD scores
    std::string assoc_pheno, assoc_covar;   // --gpca-assoc-pheno FILE (turns the association scan on), --gpca-assoc-covar FILE
    bool have_assoc_pcs = false, have_assoc_vif = false;
    bool assoc_logistic = false;      // --gpca-assoc-logistic: binary trait columns go through the logistic score scan
    int64_t assoc_pcs = 0;            // --gpca-assoc-pcs P [default: every column of the scores]
    double assoc_vif = 50.0;          // --gpca-assoc-vif X
    bool assoc_spa = false;           // --gpca-assoc-spa: the saddle-point correction of the logistic score scan
    bool have_assoc_spa_z = false;
    double assoc_spa_z = 2.0;         // --gpca-assoc-spa-z X
    bool assoc_firth = false;         // --gpca-assoc-firth: the approximate Firth correction of the logistic score scan
    bool have_assoc_firth_z = false;
    double assoc_firth_z = 1.959964;  // --gpca-assoc-firth-z X
    std::string assoc_set_list;       // --gpca-assoc-set-list FILE: gene-level set tests after the per-SNP logistic scans
    bool have_assoc_set_max_maf = false, have_assoc_set_weights = false;
    double assoc_set_max_maf = 0.01;  // --gpca-assoc-set-max-maf X
    std::string assoc_set_weights = "beta";   // --gpca-assoc-set-weights beta|flat
    std::string qtl_pheno, qtl_covar;       // --gpca-qtl-pheno FILE (turns the many-trait QTL scan on), --gpca-qtl-covar FILE
    bool have_qtl_pcs = false, have_qtl_vif = false, have_qtl_log10p = false, have_qtl_t = false;
    int64_t qtl_pcs = 0;              // --gpca-qtl-pcs P [default: every column of the scores]
    double qtl_vif = 50.0;            // --gpca-qtl-vif X
    double qtl_log10p = 5.0;          // --gpca-qtl-log10p X
    double qtl_t = 0.0;               // --gpca-qtl-t X
    gpca_host::PhenoTable qtl_pheno_table, qtl_covar_table;       // read in main, before any work on the device
    std::string qtl_cis_pos;          // --gpca-qtl-cis-pos FILE (turns cis-QTL mapping on, after the scan)
    bool have_qtl_cis_window = false, have_qtl_cis_perm = false, have_qtl_cis_seed = false, qtl_cis_only = false;
    int64_t qtl_cis_window = 1000000; // --gpca-qtl-cis-window BP
    int64_t qtl_cis_perm = 1000;      // --gpca-qtl-cis-perm P
    int64_t qtl_cis_seed = 0;         // --gpca-qtl-cis-seed S
    std::map<std::string, std::pair<std::string, int64_t>> qtl_cis_table;     // read in main
    gpca_host::PhenoTable assoc_pheno_table, assoc_covar_table;   // read in main, before any work on the device
    bool assoc_cc_freq = false;       // --gpca-assoc-cc-freq: P.<trait>.frq.cc beside every logistic scan
    std::string within;               // --gpca-within FILE: the sample groups of --gpca-freq-strat and --gpca-fst
    bool freq_strat = false;          // --gpca-freq-strat: P.frq.strat
    bool have_fst = false, fst_variants = false;   // --gpca-fst hudson|wc: P.fst.summary; --gpca-fst-variants: P.fst.var
    std::string fst;
    gpca_host::WithinTable within_table;   // read in main, before any work on the device
    bool f2 = false;                  // --gpca-f2: P.f2.summary
    std::string fstats;               // --gpca-fstats FILE: P.fstats
    bool have_fstat_block = false;
    std::string fstat_block = "5000kb";   // --gpca-fstat-block SPEC: the jackknife blocks of --gpca-f2 and --gpca-fstats
    std::vector<gpca_host::FstatSpec> fstats_list;   // read in main, before any work on the device
    bool fstat_asked() const { return f2 || !fstats.empty(); }
    bool strat_asked() const { return freq_strat || have_fst || fstat_asked(); }
    bool sample_missing = false, het = false;      // --gpca-sample-missing: P.smiss; --gpca-het: P.het
    bool have_mind = false, have_het_sd = false;   // --gpca-mind X, --gpca-het-sd K: the sample filters, P.sampleqc.in.id / .out.id
    double mind = 0.0, het_sd = 0.0;
    bool sample_qc_asked() const { return sample_missing || het || have_mind || have_het_sd; }
    bool homozyg = false;                          // --gpca-homozyg (or any of its value flags): P.hom and P.hom.indiv
    int64_t hom_window_snp = 50, hom_window_het = 1, hom_window_missing = 5, hom_snp = 100, hom_het = -1;
    bool have_hom_het = false;
    std::string hom_threshold = "0.05";
    int64_t hom_thr_num = 1, hom_thr_den = 20;     // the threshold's exact fraction, set in main
    double hom_kb = 1000.0, hom_density = 50.0, hom_gap = 1000.0;
    bool admixture = false, admix_value_flag = false;   // --gpca-admixture K; one of its value flags was given
    int64_t admix_k = 0, admix_seed = 0, admix_max_iter = 2000;
    double admix_tol = 1e-7;
    bool admix_no_accel = false, admix_supervised = false;
    bool admix_cv = false, admix_cv_flag = false;       // --gpca-admixture-cv [V]; -cv-seed or -cv-k was given
    int64_t admix_cv_folds = 5, admix_cv_seed = 0;
    std::string admix_cv_k;                             // --gpca-admixture-cv-k A-B, as given
    std::vector<int> admix_cv_ks;                       // the Ks the cross-validation scores, ascending
};

[[noreturn]] void usage_error(const std::string& msg) {
    std::fprintf(stderr, "error: %s\n\nUsage: genomic_pca --out <OUTPUT_PREFIX> (--vcf-dir <DIR> --components <K> | --eigensnp --bed-file <BED> --ld-block-file <FILE>) [options]\n"
                         "For more information, try '--help'.\n", msg.c_str());
    std::exit(2);
}

void print_help() {
    std::puts(
        "Genomic PCA Tool from VCF or BED/LD-block files.\n\n"
        "Usage: genomic_pca [OPTIONS] --out <OUTPUT_PREFIX>\n\n"
        "Options:\n"
        "  -o, --out <OUTPUT_PREFIX>            Output file prefix.\n"
        "  -t, --threads <THREADS>              accepted for compatibility (the GPU does the work)\n"
        "      --log-level <LOG_LEVEL>          [default: Info]\n"
        "  -d, --vcf-dir <VCF_DIR>              Directory containing VCF files (required if not using --eigensnp).\n"
        "  -k, --components <COMPONENTS>        Number of principal components to compute (for VCF workflow); at most 118 here\n"
        "                                       (the sketch holds components + 10 <= 128 columns; the reference has no cap).\n"
        "      --maf <MAF>                      Minimum MAF for VCF variant filtering [default: 0.01 in VCF mode]\n"
        "      --rfit-seed <RFIT_SEED>          Seed for the randomized SVD (VCF workflow).\n"
        "      --eigensnp                       Run PCA on BED + LD block files.\n"
        "      --bed-file <BED_FILE>            Path to the BED file (required if --eigensnp is used).\n"
        "      --ld-block-file <LD_BLOCK_FILE>  Path to the LD block definition file (required if --eigensnp is used).\n"
        "      --eigensnp-sample-keep-file <F>  Optional: file listing sample IDs to keep.\n"
        "      --eigensnp-min-call-rate <X>     [default: 0.98]\n"
        "      --eigensnp-min-maf <X>           [default: 0.01]\n"
        "      --eigensnp-max-hwe-p <X>         (1.0 to disable) [default: 1e-6]\n"
        "      --eigensnp-k-global <K>          [default: 10]\n"
        "      --eigensnp-components-per-block <C>  [default: 7]\n"
        "      --eigensnp-subset-factor <X>     [default: 0.075]\n"
        "      --eigensnp-min-subset-size <N>   [default: 10000]\n"
        "      --eigensnp-max-subset-size <N>   [default: 40000]\n"
        "      --eigensnp-global-oversampling <N>  [default: 10]\n"
        "      --eigensnp-global-power-iter <N> [default: 2]\n"
        "      --eigensnp-local-oversampling <N>   [default: 10]\n"
        "      --eigensnp-local-power-iter <N>  [default: 2]\n"
        "      --eigensnp-seed <SEED>           [default: 2025]\n"
        "      --eigensnp-snp-strip-size <N>    [default: 2000]\n"
        "      --eigensnp-refine-passes <N>     [default: 1]\n"
        "      --eigensnp-collect-diagnostics\n"
        "Extensions:\n"
        "      --device <N>                     HIP device ordinal\n"
        "      --write-eigenvalues              VCF workflow: fill P.eigenvalues.tsv (the reference leaves it header-only)\n"
        "      --gpca-precision <i8|f32>        i8 = exact-integer GEMMs (default); f32 = f32 matrix cores\n"
        "      --gpca-storage <auto|int8|2bit>  HBM residency of the genotypes (auto = 2bit for a .bed of >= 1024 samples, else int8)\n"
        "      --gpca-stream <auto|on|off>      walk the .bed out of core (auto = when it does not fit the device)\n"
        "      --gpca-panel-rows <N>            SNP rows per panel for --gpca-stream (0 = engine default)\n"
        "      --gpca-rfit-power-iters <N>      VCF workflow: power iterations of the randomized PCA [default: 2]\n"
        "      --gpca-eigensnp-local-stage      run the multi-stage algorithm of the --eigensnp-* local / refine flags instead of\n"
        "                                       one global randomized PCA over all blocks (the default)\n"
        "      --gpca-save-model                EigenSNP workflow: also write P.eigensnp.model.tsv (per PCA SNP: alleles, mean, s.d.,\n"
        "                                       loadings) for --gpca-project-model\n"
        "      --gpca-project-model <MODEL>     project the samples of --bed-file onto the PCs of MODEL (matched by variant ID, allele\n"
        "                                       flips handled, missing calls mean-imputed) -> P.projected.pca.tsv\n"
        "      --gpca-make-grm                  EigenSNP workflow: also write the genetic relationship matrix of the kept SNPs in\n"
        "                                       GCTA's binary layout (P.grm.bin, P.grm.N.bin, P.grm.id).  Each entry is (1/K) sum of\n"
        "                                       Z_j Z_k over the K kept SNPs, missing calls at 0: the divisor is K for every pair, not\n"
        "                                       GCTA's per-pair count, and GCTA's GRM formula is not claimed; P.grm.N.bin holds the\n"
        "                                       SNPs where both samples are observed\n"
        "      --gpca-grm-scaling <S>           --gpca-make-grm: standardized ((g - mean) / s.d., the matrix the PCA factorises) or\n"
        "                                       centred (g - mean) [default: standardized]\n"
        "      --gpca-ld-score <WINDOW>         EigenSNP workflow: after the PCA outputs, the LD score of every SNP that passes the SNP QC:\n"
        "                                       L2 = 1 + the sum of the bias-adjusted unphased r^2 with the SNPs of its chromosome at most\n"
        "                                       WINDOW away on both sides (the grammar of --gpca-indep-pairwise's WINDOW; 1000kb is the\n"
        "                                       recommendation), summed on the device -> P.l2.ldscore (CHR SNP BP L2), P.l2.M, P.l2.M_5_50.\n"
        "                                       Every sample enters, relatives and samples that fail the sample QC included.  Needs the\n"
        "                                       matrix resident on the device\n"
        "      --gpca-assoc-ldsc                --gpca-ld-score and --gpca-assoc-pheno: LD-score regression of every trait's scan statistics\n"
        "                                       (T_STAT^2 or Z_STAT^2) on the LD scores, 200 jackknife blocks -> P.ldsc.summary.  The intercept\n"
        "                                       measures confounding, H2 the SNP heritability (case / control: on the observed scale)\n"
        "      --gpca-indep-pairwise <WINDOW> <R2>  EigenSNP workflow: prune SNPs in linkage disequilibrium before the GRM, KING and the PCA\n"
        "                                       (plink's --indep-pairwise, step 1).  WINDOW = a variant count such as 50 or a span such as\n"
        "                                       250kb; 0 < R2 < 1.  Of a pair of kept SNPs with unphased r^2 > R2 the one with the smaller\n"
        "                                       minor-allele frequency leaves (ties: the later one) -> P.prune.in / P.prune.out.  Needs the\n"
        "                                       matrix resident on the device\n"
        "      --gpca-make-king                 EigenSNP workflow: also write the KING-robust kinship of every sample pair over the\n"
        "                                       kept SNPs to P.kin0 (#FID1 IID1 FID2 IID2 NSNP HETHET IBS0 KINSHIP, ID1 the earlier\n"
        "                                       sample in .fam order)\n"
        "      --gpca-king-table-filter <X>     --gpca-make-king: write only the pairs with kinship >= X\n"
        "      --gpca-king-cutoff <X>           EigenSNP workflow: drop related samples before the PCA (0 < X < 0.5; 0.0884 = second\n"
        "                                       degree).  While a pair with KING-robust kinship > X remains, the sample with the most\n"
        "                                       such partners leaves (ties: the later one in .fam order) -> P.king.cutoff.in.id / .out.id.\n"
        "                                       The PCs are fitted on the in-set and every sample is projected onto them; SNP QC, means\n"
        "                                       and s.d. stay over all samples\n"
        "      --gpca-make-pcrelate <P>         EigenSNP workflow: also write the PC-Relate kinship of every sample pair over the kept\n"
        "                                       SNPs, adjusted for the first P PCs of the scores this run writes (0 <= P <=\n"
        "                                       --eigensnp-k-global, at most 32; 0 = the homogeneous estimator), to P.pcrelate.kin\n"
        "                                       (#FID1 IID1 FID2 IID2 NSNP KINSHIP, ID1 the earlier sample in .fam order) and the\n"
        "                                       inbreeding coefficients to P.pcrelate.inbreed (#FID IID NSNP F).  With --gpca-king-cutoff\n"
        "                                       the regression is fitted on the in-set, otherwise on every sample.  Needs the matrix\n"
        "                                       resident on the device\n"
        "      --gpca-pcrelate-maf-bound <T>    --gpca-make-pcrelate: an entry counts when its individual-specific allele frequency\n"
        "                                       lies in (T, 1 - T); 0 <= T < 0.5 [default: 0.01]\n"
        "      --gpca-pcrelate-table-filter <X> --gpca-make-pcrelate: write only the pairs with kinship >= X (P.pcrelate.inbreed stays whole)\n"
        "      --gpca-assoc-pheno <FILE>        EigenSNP workflow: after everything else is written, test every SNP that passes the SNP QC\n"
        "                                       (call rate, MAF, HWE; the LD blocks and --gpca-indep-pairwise shape the PCA, not the\n"
        "                                       test set) against every trait column of FILE (header `FID IID name...`, NA = missing) by\n"
        "                                       least squares with the PCs as covariates, a missing call imputed to the SNP's mean ->\n"
        "                                       P.<trait>.assoc.linear (#CHROM POS ID A1 OBS_CT A1_FREQ BETA SE T_STAT LOG10P).  A sample\n"
        "                                       counts when every trait and covariate is present for it and, with --gpca-king-cutoff,\n"
        "                                       it is in the in-set.  Needs the matrix resident on the device; traits + PCs +\n"
        "                                       covariates <= 64\n"
        "      --gpca-assoc-logistic            --gpca-assoc-pheno: a trait column whose present values are exactly {0, 1} (1 = case) or\n"
        "                                       {1, 2} (plink's coding, 2 = case) gets the logistic score test (the null model fitted\n"
        "                                       once per trait; --gpca-assoc-spa adds the saddle-point correction, --gpca-assoc-firth the\n"
        "                                       approximate Firth correction)\n"
        "                                       -> P.<trait>.assoc.logistic (#CHROM POS ID A1 OBS_CT A1_FREQ BETA SE Z_STAT LOG10P); the\n"
        "                                       other columns go through the linear scan as without the flag.  PCs + covariates + 3 <= 64\n"
        "      --gpca-assoc-spa                 --gpca-assoc-logistic: the saddle-point correction (SPA, as SAIGE and regenie --spa) of\n"
        "                                       every test with |Z_STAT| >= the cutoff: LOG10P then comes from the saddle-point\n"
        "                                       approximation of the score's null distribution, which a rare variant in an unbalanced\n"
        "                                       trait needs, and a column SPA says Y (corrected), N (below the cutoff: the normal value)\n"
        "                                       or F (the correction did not converge: the normal value); BETA, SE and Z_STAT stay the\n"
        "                                       score test's\n"
        "      --gpca-assoc-spa-z <X>           --gpca-assoc-spa: the cutoff, at least 0.5, or inf for no correction [default: 2]\n"
        "      --gpca-assoc-firth               --gpca-assoc-logistic: the approximate Firth correction (as regenie --firth --approx) of\n"
        "                                       every test with |Z_STAT| >= the cutoff: one coefficient on the covariate-adjusted\n"
        "                                       genotype by Firth's penalised likelihood, the null model as offset.  BETA, SE and LOG10P\n"
        "                                       are then Firth's (finite where every carrier is a case), Z_STAT stays the score test's,\n"
        "                                       and a column FIRTH says Y (corrected), N (below the cutoff) or F (the fit failed: the\n"
        "                                       score test's values).  Not together with --gpca-assoc-spa\n"
        "      --gpca-assoc-firth-z <X>         --gpca-assoc-firth: the cutoff, at least 0, or inf for no correction [default: 1.959964]\n"
        "      --gpca-assoc-set-list <FILE>     --gpca-assoc-logistic: gene-level set tests after the per-SNP scans.  FILE is regenie's set\n"
        "                                       list, one set per line: NAME CHROM POS ID1,ID2,... (IDs that the SNP QC removed are\n"
        "                                       dropped).  Every case / control trait gets P.<trait>.assoc.set (#SET CHROM POS N_VAR\n"
        "                                       N_USED BURDEN_BETA BURDEN_SE BURDEN_Z BURDEN_LOG10P SKAT_Q SKAT_LOG10P SKAT): a weighted\n"
        "                                       burden test and SKAT (its p-value by Kuonen's saddle point: SKAT = Y; N = the bulk\n"
        "                                       approximation, F = the saddle point failed) from the covariance of the set's scores\n"
        "                                       under the null model.  A set with no variant left, or with more than 128, gets NA\n"
        "      --gpca-assoc-set-max-maf <X>     --gpca-assoc-set-list: a listed variant enters its set when its minor-allele frequency\n"
        "                                       over the included observed calls is at most X, 0 < X <= 0.5 [default: 0.01]\n"
        "      --gpca-assoc-set-weights <KIND>  --gpca-assoc-set-list: beta = Beta(maf; 1, 25) weights, flat = 1 [default: beta]\n"
        "      --gpca-assoc-cc-freq             --gpca-assoc-logistic: the genotype counts and A1 frequencies of every SNP among the\n"
        "                                       controls and the cases of every case / control trait, over the scan's include set ->\n"
        "                                       <out>.<trait>.frq.cc (the .frq.strat format with the groups CTRL and CASE)\n"
        "      --gpca-within <FILE>             --eigensnp: the sample groups of --gpca-freq-strat and --gpca-fst, a table `FID IID GROUP`\n"
        "                                       with that header; NA = no group; at most 64 groups\n"
        "      --gpca-freq-strat                --gpca-within: the genotype counts, A1 frequency and HWE p-value of every SNP that passes\n"
        "                                       the SNP QC inside every group -> <out>.frq.strat\n"
        "      --gpca-fst <METHOD>              --gpca-within: Fst between every pair of groups over the SNPs that pass the SNP QC, hudson\n"
        "                                       (Bhatia et al. 2013) or wc (Weir and Cockerham 1984; with more than two groups also\n"
        "                                       jointly) -> <out>.fst.summary\n"
        "      --gpca-fst-variants              --gpca-fst: also the per-SNP terms -> <out>.fst.var\n"
        "      --gpca-f2                        --gpca-within: the unbiased f2 of every pair of groups over the SNPs that pass the SNP QC,\n"
        "                                       with its weighted block-jackknife standard error -> <out>.f2.summary\n"
        "      --gpca-fstats <FILE>             --gpca-within: the statistics FILE lists, one per line: `f2 A B`, `f3 C A B` (C is the\n"
        "                                       target) or `f4 A B C D` with group names -> <out>.fstats (estimate, jackknife SE, Z)\n"
        "      --gpca-fstat-block <SPEC>        --gpca-f2 / --gpca-fstats: the jackknife blocks, a variant count such as 500 or a span\n"
        "                                       such as 5000kb; a block ends at every change of chromosome [default: 5000kb]\n"
        "      --gpca-sample-missing            --eigensnp: the missing calls of every sample over the SNPs that pass the SNP QC ->\n"
        "                                       <out>.smiss (#FID IID MISSING_CT OBS_CT F_MISS)\n"
        "      --gpca-het                       --eigensnp: the observed and expected homozygous calls and the inbreeding coefficient F of\n"
        "                                       every sample over the SNPs that pass the SNP QC (plink --het, allele frequencies from all\n"
        "                                       samples) -> <out>.het (#FID IID O_HOM E_HOM OBS_CT F)\n"
        "      --gpca-mind <X>                  --eigensnp: drop a sample from the fit, PC-Relate's training set and the scans when more\n"
        "                                       than X of its calls are missing (0 <= X < 1) -> <out>.sampleqc.in.id / .out.id; every\n"
        "                                       sample is still projected\n"
        "      --gpca-het-sd <K>                --eigensnp: drop a sample whose F lies more than K standard deviations from the mean F of\n"
        "                                       the samples that pass --gpca-mind (K > 0; one round) -> <out>.sampleqc.in.id / .out.id\n"
        "      --gpca-homozyg                   --eigensnp: runs of homozygosity of every sample over the SNPs that pass the SNP QC (plink\n"
        "                                       --homozyg's sliding window) -> <out>.hom (#FID IID CHROM SNP1 SNP2 POS1 POS2 KB NSNP DENSITY\n"
        "                                       PHOM PHET) and <out>.hom.indiv (#FID IID NSEG KB KBAVG FROH); any flag below implies it\n"
        "      --gpca-homozyg-window-snp <W>    the scanning window in SNPs (1 .. 64) [default: 50]\n"
        "      --gpca-homozyg-window-het <H>    het calls a window may hold and still be a hit (0 .. W) [default: 1]\n"
        "      --gpca-homozyg-window-missing <M>  missing calls a window may hold and still be a hit (0 .. W) [default: 5]\n"
        "      --gpca-homozyg-window-threshold <X>  the share of hits among the windows over a SNP that puts it in a run, a decimal\n"
        "                                       number in [0, 1] taken as its exact fraction [default: 0.05]\n"
        "      --gpca-homozyg-snp <N>           SNPs a run needs at least [default: 100]\n"
        "      --gpca-homozyg-kb <X>            kb a run spans at least [default: 1000]\n"
        "      --gpca-homozyg-density <X>       kb per SNP a run holds at most [default: 50]\n"
        "      --gpca-homozyg-gap <X>           a gap of more than X kb between two SNPs ends a run [default: 1000]\n"
        "      --gpca-homozyg-het <N>           het calls a run holds at most [default: no limit]\n"
        "      --gpca-admixture <K>             --eigensnp: admixture proportions of every sample in K ancestral populations (1 .. 16), the\n"
        "                                       ADMIXTURE model fitted by accelerated EM over the SNPs the PCA is fitted on; samples outside\n"
        "                                       the KING in-set or failing the sample QC get proportions without shaping the frequencies\n"
        "                                       -> <out>.K.Q, .Q.id, .P, .P.id and .admix.log\n"
        "      --gpca-admixture-seed <S>        the seed of the starting point [default: 0]\n"
        "      --gpca-admixture-max-iter <N>    EM steps at most [default: 2000]\n"
        "      --gpca-admixture-tol <X>         stop when a cycle gains less than X times the log-likelihood [default: 1e-7]\n"
        "      --gpca-admixture-no-accel        plain EM steps, without the SQUAREM acceleration\n"
        "      --gpca-admixture-cv [V]          --gpca-admixture: the V-fold cross-validation error of the fit (2 .. 64): a random V-th of the\n"
        "                                       observed calls is hidden from a refit and scored by its binomial deviance, once per fold\n"
        "                                       -> <out>.admix.cv [default V: 5]\n"
        "      --gpca-admixture-cv-seed <S>     the seed of the folds [default: 0]\n"
        "      --gpca-admixture-cv-k <A-B>      --gpca-admixture-cv: also score every K of A .. B (1 <= A <= B <= 16) into <out>.admix.cv,\n"
        "                                       to choose K\n"
        "      --gpca-admixture-supervised      the samples with a group in --gpca-within are references of known ancestry: K must be the\n"
        "                                       number of groups, and column k of the result is group k\n"
        "      --gpca-assoc-pcs <P>             --gpca-assoc-pheno: the first P columns of the scores this run writes are covariates\n"
        "                                       (0 <= P <= --eigensnp-k-global) [default: every column]\n"
        "      --gpca-assoc-covar <FILE>        --gpca-assoc-pheno: further covariates, a table in the format of the phenotype file\n"
        "      --gpca-qtl-pheno <FILE>          EigenSNP workflow: after everything else is written, test every SNP that passes the SNP QC\n"
        "                                       against every column of FILE (`FID IID name...`, up to 2^20 traits) in one wide pass on\n"
        "                                       the GPU; the pairs beyond the threshold go to <out>.qtl.hits, the best SNP of every trait\n"
        "                                       to <out>.qtl.best\n"
        "      --gpca-qtl-pcs <P>               --gpca-qtl-pheno: the first P columns of the scores this run writes are covariates\n"
        "      --gpca-qtl-covar <FILE>          --gpca-qtl-pheno: further covariates (at most 63 with the PCs)\n"
        "      --gpca-qtl-log10p <X>            --gpca-qtl-pheno: keep the pairs with -log10 p >= X [default: 5]\n"
        "      --gpca-qtl-t <X>                 --gpca-qtl-pheno: keep the pairs with |t| >= X instead\n"
        "      --gpca-qtl-vif <X>               --gpca-qtl-pheno: a SNP whose variance inflation exceeds X is not tested [default: 50]\n"
        "      --gpca-qtl-cis-pos <FILE>        --gpca-qtl-pheno: cis-QTL mapping after the scan: FILE is a `TRAIT CHROM POS` table; every trait\n"
        "                                       with a position is tested against the SNPs within the window around it, with a permutation\n"
        "                                       null and its beta approximation, into <out>.qtl.cis\n"
        "      --gpca-qtl-cis-window <BP>       --gpca-qtl-cis-pos: |SNP - POS| <= BP [default: 1000000]\n"
        "      --gpca-qtl-cis-perm <P>          --gpca-qtl-cis-pos: permutations of the traits [default: 1000; 0 = nominal only]\n"
        "      --gpca-qtl-cis-seed <S>          --gpca-qtl-cis-pos: the seed of the permutation table [default: 0]\n"
        "      --gpca-qtl-cis-only              --gpca-qtl-cis-pos: skip the scan of every SNP against every trait\n"
        "      --gpca-assoc-vif <X>             --gpca-assoc-pheno: a SNP whose variance inflation against the covariates exceeds X gets\n"
        "                                       NA (plink's --vif) [default: 50]\n"
        "  -h, --help                           Print help");
}

int64_t to_i64(const std::string& flag, const std::string& v) {
    try { size_t n = 0; const long long x = std::stoll(v, &n); if (n != v.size()) throw 1; return x; }
    catch (...) { usage_error("invalid value '" + v + "' for '" + flag + "'"); }
}
uint64_t to_u64(const std::string& flag, const std::string& v) {
    try { size_t n = 0; if (!v.empty() && v[0] == '-') throw 1; const unsigned long long x = std::stoull(v, &n); if (n != v.size()) throw 1; return x; }
    catch (...) { usage_error("invalid value '" + v + "' for '" + flag + "'"); }
}
double to_f64(const std::string& flag, const std::string& v) {
    try { size_t n = 0; const double x = std::stod(v, &n); if (n != v.size()) throw 1; return x; }
    catch (...) { usage_error("invalid value '" + v + "' for '" + flag + "'"); }
}

Args parse(int argc, char** argv) {
    Args a;
    for (int i = 1; i < argc; ++i) {
        std::string f = argv[i], inline_val;
        bool has_inline = false;
        if (f.compare(0, 2, "--") == 0) { const size_t eq = f.find('='); if (eq != std::string::npos) { inline_val = f.substr(eq + 1); f = f.substr(0, eq); has_inline = true; } }
        auto val = [&]() -> std::string {
            if (has_inline) return inline_val;
            if (i + 1 >= argc) usage_error("a value is required for '" + f + "' but none was supplied");
            return argv[++i];
        };
        if (f == "-h" || f == "--help") { print_help(); std::exit(0); }
        else if (f == "-o" || f == "--out") a.output_prefix = val();
        else if (f == "-t" || f == "--threads") a.threads = to_i64(f, val());
        else if (f == "--log-level") a.log_level = val();
        else if (f == "-d" || f == "--vcf-dir") a.vcf_dir = val();
        else if (f == "-k" || f == "--components") { a.components = to_i64(f, val()); a.have_components = true; if (a.components < 0) usage_error("invalid value for '--components'"); }
        else if (f == "--maf") { a.maf = to_f64(f, val()); a.have_maf = true; }
        else if (f == "--rfit-seed") { a.rfit_seed = to_u64(f, val()); a.have_seed = true; }
        else if (f == "--eigensnp") a.eigensnp = true;
        else if (f == "--bed-file") a.bed_file = val();
        else if (f == "--ld-block-file") a.ld_block_file = val();
        else if (f == "--eigensnp-sample-keep-file") a.sample_keep_file = val();
        else if (f == "--eigensnp-min-call-rate") a.min_call_rate = to_f64(f, val());
        else if (f == "--eigensnp-min-maf") a.min_maf = to_f64(f, val());
        else if (f == "--eigensnp-max-hwe-p") a.max_hwe_p = to_f64(f, val());
        else if (f == "--eigensnp-k-global") a.k_global = to_i64(f, val());
        else if (f == "--eigensnp-components-per-block") a.components_per_block = to_i64(f, val());
        else if (f == "--eigensnp-subset-factor") a.subset_factor = to_f64(f, val());
        else if (f == "--eigensnp-min-subset-size") a.min_subset = to_i64(f, val());
        else if (f == "--eigensnp-max-subset-size") a.max_subset = to_i64(f, val());
        else if (f == "--eigensnp-global-oversampling") a.global_oversampling = to_i64(f, val());
        else if (f == "--eigensnp-global-power-iter") a.global_power_iter = to_i64(f, val());
        else if (f == "--eigensnp-local-oversampling") a.local_oversampling = to_i64(f, val());
        else if (f == "--eigensnp-local-power-iter") a.local_power_iter = to_i64(f, val());
        else if (f == "--eigensnp-seed") a.seed = to_u64(f, val());
        else if (f == "--eigensnp-snp-strip-size") a.strip_size = to_i64(f, val());
        else if (f == "--eigensnp-refine-passes") a.refine_passes = to_i64(f, val());
        else if (f == "--eigensnp-collect-diagnostics") a.collect_diagnostics = true;
        else if (f == "--device") a.device = (int)to_i64(f, val());
        else if (f == "--write-eigenvalues") a.write_eigenvalues = true;
        else if (f == "--gpca-precision") { a.precision = val(); if (a.precision != "i8" && a.precision != "f32") usage_error("invalid value '" + a.precision + "' for '--gpca-precision' (i8, f32)"); }
        else if (f == "--gpca-storage") { a.storage = val(); if (a.storage != "auto" && a.storage != "int8" && a.storage != "2bit") usage_error("invalid value '" + a.storage + "' for '--gpca-storage' (auto, int8, 2bit)"); }
        else if (f == "--gpca-stream") { a.stream = val(); if (a.stream != "auto" && a.stream != "on" && a.stream != "off") usage_error("invalid value '" + a.stream + "' for '--gpca-stream' (auto, on, off)"); }
        else if (f == "--gpca-panel-rows") a.panel_rows = to_i64(f, val());
        else if (f == "--gpca-rfit-power-iters") a.rfit_power_iters = to_i64(f, val());
        else if (f == "--gpca-eigensnp-local-stage") a.local_stage = true;
        else if (f == "--gpca-save-model") a.save_model = true;
        else if (f == "--gpca-project-model") a.project_model = val();
        else if (f == "--gpca-make-grm") a.make_grm = true;
        else if (f == "--gpca-grm-scaling") { a.grm_scaling = val(); if (a.grm_scaling != "standardized" && a.grm_scaling != "centred") usage_error("invalid value '" + a.grm_scaling + "' for '--gpca-grm-scaling' (standardized, centred)"); }
        else if (f == "--gpca-make-king") a.make_king = true;
        else if (f == "--gpca-king-table-filter") { a.king_filter = to_f64(f, val()); a.have_king_filter = true; }
        else if (f == "--gpca-king-cutoff") { a.king_cutoff = to_f64(f, val()); a.have_king_cutoff = true; }
        else if (f == "--gpca-make-pcrelate") { a.pcrelate_pcs = to_i64(f, val()); a.make_pcrelate = true; }
        else if (f == "--gpca-pcrelate-maf-bound") { a.pcrelate_tau = to_f64(f, val()); a.have_pcrelate_tau = true; }
        else if (f == "--gpca-pcrelate-table-filter") { a.pcrelate_filter = to_f64(f, val()); a.have_pcrelate_filter = true; }
        else if (f == "--gpca-assoc-pheno") a.assoc_pheno = val();
        else if (f == "--gpca-assoc-covar") a.assoc_covar = val();
        else if (f == "--gpca-assoc-logistic") a.assoc_logistic = true;
        else if (f == "--gpca-assoc-spa") a.assoc_spa = true;
        else if (f == "--gpca-assoc-spa-z") { a.assoc_spa_z = to_f64(f, val()); a.have_assoc_spa_z = true; }
        else if (f == "--gpca-assoc-firth") a.assoc_firth = true;
        else if (f == "--gpca-assoc-firth-z") { a.assoc_firth_z = to_f64(f, val()); a.have_assoc_firth_z = true; }
        else if (f == "--gpca-assoc-set-list") a.assoc_set_list = val();
        else if (f == "--gpca-assoc-set-max-maf") { a.assoc_set_max_maf = to_f64(f, val()); a.have_assoc_set_max_maf = true; }
        else if (f == "--gpca-assoc-set-weights") { a.assoc_set_weights = val(); a.have_assoc_set_weights = true; }
        else if (f == "--gpca-assoc-cc-freq") a.assoc_cc_freq = true;
        else if (f == "--gpca-within") a.within = val();
        else if (f == "--gpca-freq-strat") a.freq_strat = true;
        else if (f == "--gpca-fst") { a.fst = val(); a.have_fst = true; }
        else if (f == "--gpca-fst-variants") a.fst_variants = true;
        else if (f == "--gpca-f2") a.f2 = true;
        else if (f == "--gpca-fstats") a.fstats = val();
        else if (f == "--gpca-fstat-block") { a.fstat_block = val(); a.have_fstat_block = true; }
        else if (f == "--gpca-sample-missing") a.sample_missing = true;
        else if (f == "--gpca-het") a.het = true;
        else if (f == "--gpca-mind") { a.mind = to_f64(f, val()); a.have_mind = true; }
        else if (f == "--gpca-het-sd") { a.het_sd = to_f64(f, val()); a.have_het_sd = true; }
        else if (f == "--gpca-admixture") { a.admix_k = to_i64(f, val()); a.admixture = true; }
        else if (f == "--gpca-admixture-seed") { a.admix_seed = to_i64(f, val()); a.admix_value_flag = true; }
        else if (f == "--gpca-admixture-max-iter") { a.admix_max_iter = to_i64(f, val()); a.admix_value_flag = true; }
        else if (f == "--gpca-admixture-tol") { a.admix_tol = to_f64(f, val()); a.admix_value_flag = true; }
        else if (f == "--gpca-admixture-no-accel") { a.admix_no_accel = true; a.admix_value_flag = true; }
        else if (f == "--gpca-admixture-supervised") { a.admix_supervised = true; a.admix_value_flag = true; }
        else if (f == "--gpca-admixture-cv") {                                            // the value is optional: taken unless a flag follows
            a.admix_cv = true;
            const bool next = i + 1 < argc && (argv[i + 1][0] != '-' || (argv[i + 1][1] >= '0' && argv[i + 1][1] <= '9'));
            if (has_inline || next) a.admix_cv_folds = to_i64(f, val());
        }
        else if (f == "--gpca-admixture-cv-seed") { a.admix_cv_seed = to_i64(f, val()); a.admix_cv_flag = true; }
        else if (f == "--gpca-admixture-cv-k") { a.admix_cv_k = val(); a.admix_cv_flag = true; if (a.admix_cv_k.empty()) a.admix_cv_k = " "; }
        else if (f == "--gpca-homozyg") a.homozyg = true;
        else if (f == "--gpca-homozyg-window-snp") { a.hom_window_snp = to_i64(f, val()); a.homozyg = true; }
        else if (f == "--gpca-homozyg-window-het") { a.hom_window_het = to_i64(f, val()); a.homozyg = true; }
        else if (f == "--gpca-homozyg-window-missing") { a.hom_window_missing = to_i64(f, val()); a.homozyg = true; }
        else if (f == "--gpca-homozyg-window-threshold") { a.hom_threshold = val(); a.homozyg = true; }
        else if (f == "--gpca-homozyg-snp") { a.hom_snp = to_i64(f, val()); a.homozyg = true; }
        else if (f == "--gpca-homozyg-kb") { a.hom_kb = to_f64(f, val()); a.homozyg = true; }
        else if (f == "--gpca-homozyg-density") { a.hom_density = to_f64(f, val()); a.homozyg = true; }
        else if (f == "--gpca-homozyg-gap") { a.hom_gap = to_f64(f, val()); a.homozyg = true; }
        else if (f == "--gpca-homozyg-het") { a.hom_het = to_i64(f, val()); a.have_hom_het = true; a.homozyg = true; }
        else if (f == "--gpca-qtl-pheno") a.qtl_pheno = val();
        else if (f == "--gpca-qtl-covar") a.qtl_covar = val();
        else if (f == "--gpca-qtl-pcs") { a.qtl_pcs = to_i64(f, val()); a.have_qtl_pcs = true; }
        else if (f == "--gpca-qtl-vif") { a.qtl_vif = to_f64(f, val()); a.have_qtl_vif = true; }
        else if (f == "--gpca-qtl-log10p") { a.qtl_log10p = to_f64(f, val()); a.have_qtl_log10p = true; }
        else if (f == "--gpca-qtl-t") { a.qtl_t = to_f64(f, val()); a.have_qtl_t = true; }
        else if (f == "--gpca-qtl-cis-pos") a.qtl_cis_pos = val();
        else if (f == "--gpca-qtl-cis-window") { a.qtl_cis_window = to_i64(f, val()); a.have_qtl_cis_window = true; }
        else if (f == "--gpca-qtl-cis-perm") { a.qtl_cis_perm = to_i64(f, val()); a.have_qtl_cis_perm = true; }
        else if (f == "--gpca-qtl-cis-seed") { a.qtl_cis_seed = to_i64(f, val()); a.have_qtl_cis_seed = true; }
        else if (f == "--gpca-qtl-cis-only") a.qtl_cis_only = true;
        else if (f == "--gpca-assoc-pcs") { a.assoc_pcs = to_i64(f, val()); a.have_assoc_pcs = true; }
        else if (f == "--gpca-assoc-vif") { a.assoc_vif = to_f64(f, val()); a.have_assoc_vif = true; }
        else if (f == "--gpca-ld-score") a.ld_score = val();
        else if (f == "--gpca-assoc-ldsc") a.assoc_ldsc = true;
        else if (f == "--gpca-indep-pairwise") {
            a.indep_window = val();
            if (i + 1 >= argc) usage_error("two values (WINDOW R2) are required for '" + f + "'");
            a.indep_r2_text = argv[++i]; a.have_indep = true;
        }
        else usage_error("unexpected argument '" + f + "' found");
    }
    if (a.output_prefix.empty()) usage_error("the following required arguments were not provided:\n  --out <OUTPUT_PREFIX>");
    return a;
}

void logmsg(const std::string& m) { std::fprintf(stderr, "[genomic_pca] %s\n", m.c_str()); }

double seconds_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

int engine_precision(const Args& a) { return a.precision == "i8" ? GPCA_PREC_I8_EXACT : GPCA_PREC_F32_MFMA; }
// storage "auto": a .bed of >= 1 024 samples stays in its own 2-bit form (a quarter of the HBM, faster packed kernels there);
// narrower matrices and VCF input are int8 (cli.py:_engine_modes)
int engine_storage(Args& a, int64_t bed_samples = 0) {
    if (a.storage == "auto") a.storage = bed_samples >= 1024 ? "2bit" : "int8";
    return a.storage == "2bit" ? GPCA_STORE_2BIT : GPCA_STORE_INT8;
}

// ------------------------------------------------------------------------------------------------ VCF workflow
int run_vcf_workflow(Args a) {
    if (a.vcf_dir.empty() || !a.have_components) {
        std::fprintf(stderr, "error: --vcf-dir and --components are required unless --eigensnp is given\n");
        return 2;
    }
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::string> files;
    if (DIR* d = opendir(a.vcf_dir.c_str())) {
        while (dirent* e = readdir(d)) {
            const std::string n = e->d_name;
            if (gpca_host::ends_with(n, ".vcf") || gpca_host::ends_with(n, ".vcf.gz")) files.push_back(a.vcf_dir + "/" + n);
        }
        closedir(d);
    }
    std::sort(files.begin(), files.end());
    if (files.empty()) { std::fprintf(stderr, "No VCF files found in %s\n", a.vcf_dir.c_str()); return 1; }          // main.rs:153-155
    gpca_host::VcfData v;
    for (size_t i = 0; i < files.size(); ++i) gpca_host::read_vcf(files[i], a.have_maf ? a.maf : 0.01, v, i == 0);
    const int64_t n_samples = (int64_t)v.samples.size(), n_variants = (int64_t)v.variant_ids.size();
    char buf[256];
    std::snprintf(buf, sizeof buf, "%zu VCF files, %lld variants x %lld samples in %.2fs", files.size(), (long long)n_variants, (long long)n_samples, seconds_since(t0));
    logmsg(buf);
    if (n_variants == 0) { std::fprintf(stderr, "No variants available to build matrix.\n"); return 1; }              // vcf.rs:321-323
    gpca::PCA model(a.device, engine_precision(a), engine_storage(a));
    model.rfit(v.dosages.data(), n_variants, n_samples, (int)a.components, 10, a.have_seed ? a.rfit_seed : 0, (int)a.rfit_power_iters);          // main.rs:636-656
    const std::vector<double> pcs = model.transform();
    gpca_host::ensure_parent(a.output_prefix);
    gpca_host::write_principal_components(a.output_prefix, "vcf.pca.tsv", v.samples, pcs.data(), n_samples, model.components());   // main.rs:231
    gpca_host::write_eigenvalues(a.output_prefix, a.write_eigenvalues ? model.explained_variance() : std::vector<double>());        // main.rs:232, 676
    std::snprintf(buf, sizeof buf, "VCF workflow done in %.2fs", seconds_since(t0));
    logmsg(buf);
    return 0;
}

// ------------------------------------------------------------------------------------------------ EigenSNP workflow
struct KeptColumns {            // host-side decode of the kept sample columns (a sample keep file): the panel source of that case
    const gpca_host::PlinkFileset* fs;
    std::vector<int64_t> cols;
};
extern "C" int fill_kept_columns(void* user, int64_t row0, int64_t rows, void* dst, int64_t ld) {
    static const int8_t lut[4] = {2, -127, 1, 0};                // count_a1 (prepare.rs:622-629)
    const KeptColumns* k = static_cast<const KeptColumns*>(user);
    int8_t* out = static_cast<int8_t*>(dst);
    for (int64_t r = 0; r < rows; ++r) {
        const uint8_t* src = k->fs->bed_rows + (row0 + r) * k->fs->bytes_per_row;
        int8_t* o = out + r * ld;
        for (size_t c = 0; c < k->cols.size(); ++c) { const int64_t s = k->cols[c]; o[c] = lut[(src[s >> 2] >> (2 * (s & 3))) & 3]; }
    }
    return 0;
}
// The .bed payload into the engine: resident, or -- when it does not fit the device, or on request -- out of core with the
// HBM panel cache on (cli.py:_load_bed; the reference pulls strips through the accessor on every pass, main.rs:322).  Returns true
// when the matrix is walked out of core.
bool load_bed(gpca::Engine& eng, const Args& a, const gpca_host::PlinkFileset& fs, KeptColumns* kept) {
    gpca_panel_source src;
    std::memset(&src, 0, sizeof src);
    const int64_t n_samples = kept ? (int64_t)kept->cols.size() : fs.n_samples;
    if (kept) { src.kind = GPCA_PANEL_HOST_I8; src.fill = fill_kept_columns; src.user = kept; }
    else {   // the memory-mapped payload itself is the source: the library's copy threads stage its panels, no callback
        src.kind = GPCA_PANEL_MAPPED_BED; src.user = const_cast<uint8_t*>(fs.bed_rows); src.host_ld = fs.bytes_per_row;
    }
    std::string mode = a.stream;
    if (mode == "auto") {
        // resident needs the matrix (1 B or 0.25 B per genotype, rows padded) plus the solver's workspace (gpca.h,
        // gpca_get_device_memory): a load that fits with nothing to spare would only fail later, in gpca_rsvd
        int64_t free_b = eng.device_memory().first;
        if (const char* e = std::getenv("GPCA_CLI_FREE_BYTES")) free_b = std::atoll(e);       // (test hook: pretend the device is smaller)
        const int64_t per_row = (n_samples + 1023) / 1024 * 1024 / (a.storage == "2bit" ? 4 : 1) + 512;
        const double need = (double)fs.n_snps * (double)(per_row + 1024) + (double)n_samples * 8192.0 + 1073741824.0;
        if (need > (double)free_b) {
            char buf[200];
            std::snprintf(buf, sizeof buf, "the genotype matrix needs about %.1f GiB resident, %.1f GiB are free: walking it out of core",
                          need / 1073741824.0, (double)free_b / 1073741824.0);
            logmsg(buf);
            mode = "on";
        }
    }
    if (mode != "on") {
        try {
            if (kept) eng.load_from_source(src, fs.n_snps, n_samples);
            else eng.upload_bed2bit(fs.bed_rows, fs.n_snps, fs.n_samples);     // the memory map goes up in 256 MiB row chunks, decoded on the GPU
            return false;
        } catch (const gpca::Error& e) {
            if (mode == "off" || e.status() != GPCA_ERR_OOM) throw;
            logmsg("the genotype matrix does not fit the device: walking it out of core");
        }
    }
    eng.stream_open(src, fs.n_snps, n_samples, a.panel_rows, 3, true, -1);
    return true;
}

const char* const kPcrelateNeedsResident =
    "error: --gpca-make-pcrelate needs the genotype matrix resident on the device: the f32 sums are not associative across the panels of a "
    "matrix walked out of core\n";

const char* const kStratNeedsResident =
    "error: --gpca-within needs the genotype matrix resident on the device: the counts of a matrix walked out of core are not implemented\n";

// --gpca-freq-strat / --gpca-fst: the genotype counts of every SNP that passes the SNP QC inside every group of --gpca-within
// (gpca_group_counts), in row bands, into P.frq.strat, and Fst from them (gpca_fst_hudson / gpca_fst_wc) into P.fst.summary and
// P.fst.var.  Resets the keep mask to the QC mask (mu, sigma unchanged), which ends the fit's validity; every kept sample with a group
// counts, the KING in-set or not (cli.py:_strat).  --gpca-f2 / --gpca-fstats: the same bands through gpca_f2_blocks, whose counts serve the
// files above, the blocks from fstat_blocks over the same SNPs; gpca_fstat turns the summed blocks into P.f2.summary and P.fstats.
int run_strat(gpca::Engine& eng, const Args& a, const gpca_host::PlinkFileset& fs, const std::vector<std::string>& fids,
              const std::vector<std::string>& sample_ids, const gpca::SnpStats& st) {
    const std::vector<int32_t> labels = gpca_host::align_within(a.within_table, fids, sample_ids);
    const std::vector<std::string>& names = a.within_table.names;
    const int32_t P = (int32_t)names.size();
    eng.set_standardization(st.mu, st.sigma, st.keep);                                // every SNP that passes the SNP QC
    std::vector<int64_t> rows;
    for (size_t i = 0; i < st.keep.size(); ++i) if (st.keep[i]) rows.push_back((int64_t)i);
    gpca_host::ensure_parent(a.output_prefix);
    const size_t pairs = (size_t)P * (size_t)(P - 1) / 2;
    const bool hudson = a.have_fst && a.fst == "hudson", wc = a.have_fst && a.fst == "wc";
    std::vector<double> hud(pairs * 3, 0.0), wcp(pairs * 3, 0.0);
    double wcj[3] = {0.0, 0.0, 0.0};
    std::unique_ptr<gpca_host::FrqStratWriter> wf;
    std::unique_ptr<gpca_host::FstVarWriter> wv;
    if (a.freq_strat) wf.reset(new gpca_host::FrqStratWriter(a.output_prefix + ".frq.strat", names, gpca_hwe_chi_squared_p_value));
    if (a.have_fst && a.fst_variants) wv.reset(new gpca_host::FstVarWriter(a.output_prefix, wc, names));
    const bool fstat = a.fstat_asked(), need_counts = a.freq_strat || a.have_fst;
    std::vector<int32_t> block;
    int32_t B = 0;
    std::vector<int64_t> facc, fcnt;
    if (fstat) {
        std::vector<std::string> chrom;
        std::vector<int64_t> pos;
        for (int64_t o : rows) { chrom.push_back(fs.chromosomes[(size_t)o]); pos.push_back(fs.positions[(size_t)o]); }
        block = gpca_host::fstat_blocks(chrom, pos, a.fstat_block, B);
        facc.assign((size_t)std::max<int32_t>(B, 1) * pairs, 0); fcnt = facc;
    }
    try {
        for (const auto& b : gpca_host::group_count_bands((int64_t)rows.size(), P, (int64_t)1 << 26, fstat ? gpca_host::kF2BandRowsMax : 0)) {
            std::vector<uint32_t> c;
            if (fstat) {
                std::vector<int64_t> bacc, bcnt;
                eng.f2_blocks(labels, P, b.first, b.second, std::vector<int32_t>(block.begin() + b.first, block.begin() + b.second), B, bacc, bcnt,
                              need_counts ? &c : nullptr);
                for (size_t k = 0; k < facc.size(); ++k) { facc[k] += bacc[k]; fcnt[k] += bcnt[k]; }
            } else {
                eng.group_counts(labels, P, b.first, b.second, c);
            }
            const size_t nr = (size_t)(b.second - b.first);
            if (wf)
                for (size_t i = 0; i < nr; ++i) {
                    const size_t o = (size_t)rows[(size_t)b.first + i];
                    wf->add_row(fs.chromosomes[o], fs.positions[o], fs.variant_ids[o], fs.allele1[o], &c[i * (size_t)P * 3]);
                }
            std::vector<double> vals;                                                   // [rows][pairs][2 or 3]
            if (hudson) {
                std::vector<double> num, den;
                gpca::Engine::fst_hudson(c, P, hud, wv ? &num : nullptr, wv ? &den : nullptr);
                if (wv) {
                    vals.resize(nr * pairs * 2);
                    for (size_t k = 0; k < nr * pairs; ++k) { vals[2 * k] = num[k]; vals[2 * k + 1] = den[k]; }
                }
            } else if (wc) {
                if (wv) vals.resize(nr * pairs * 3);
                size_t q = 0;
                for (int32_t i = 1; i < P; ++i)
                    for (int32_t j = 0; j < i; ++j, ++q) {                              // r = 2 on each pair
                        std::vector<uint8_t> use((size_t)P, 0);
                        use[(size_t)j] = use[(size_t)i] = 1;
                        std::vector<double> abc;
                        gpca::Engine::fst_wc(c, P, use, &wcp[3 * q], wv ? &abc : nullptr);
                        if (wv) for (size_t r = 0; r < nr; ++r) for (int k = 0; k < 3; ++k) vals[(r * pairs + q) * 3 + (size_t)k] = abc[3 * r + (size_t)k];
                    }
                if (P > 2) gpca::Engine::fst_wc(c, P, {}, wcj, nullptr);
            }
            if (wv)
                for (size_t i = 0; i < nr; ++i) {
                    const size_t o = (size_t)rows[(size_t)b.first + i];
                    wv->add_row(fs.chromosomes[o], fs.positions[o], fs.variant_ids[o], &vals[i * pairs * (wc ? 3 : 2)]);
                }
        }
    } catch (const gpca::Error& e) {
        if (e.status() != GPCA_ERR_STATE) throw;
        std::fputs(kStratNeedsResident, stderr);
        return 1;
    }
    int64_t n_lab = 0;
    for (int32_t g : labels) n_lab += g >= 0;
    char buf[512];
    if (a.freq_strat) {
        std::snprintf(buf, sizeof buf, "genotype counts of %zu SNPs in %d groups (%lld of %zu samples), written to %s.frq.strat", rows.size(), (int)P,
                      (long long)n_lab, sample_ids.size(), a.output_prefix.c_str());
        logmsg(buf);
    }
    if (a.have_fst) {
        std::vector<double> sums = hudson ? hud : wcp;
        if (wc && P > 2) sums.insert(sums.end(), wcj, wcj + 3);
        gpca_host::write_fst_summary(a.output_prefix, wc, names, sums);
        std::snprintf(buf, sizeof buf, "%s Fst of %zu pairs of groups over %zu SNPs, written to %s.fst.summary", a.fst.c_str(), pairs, rows.size(),
                      a.output_prefix.c_str());
        logmsg(buf);
    }
    if (fstat && B >= 1) {
        if (a.f2) {
            std::vector<int32_t> quads;
            for (int32_t i = 1; i < P; ++i)
                for (int32_t j = 0; j < i; ++j) { const int32_t q[4] = {j, i, j, i}; quads.insert(quads.end(), q, q + 4); }
            gpca_host::write_f2_summary(a.output_prefix, names, gpca::Engine::fstat(facc, fcnt, B, P, quads));
            std::snprintf(buf, sizeof buf, "f2 of %zu pairs of groups over %zu SNPs in %d jackknife blocks (%s), written to %s.f2.summary", pairs, rows.size(),
                          (int)B, a.fstat_block.c_str(), a.output_prefix.c_str());
            logmsg(buf);
        }
        if (!a.fstats.empty()) {
            std::vector<int32_t> quads;
            for (const auto& s : a.fstats_list) { int32_t q[4]; gpca_host::fstat_quad(s, q); quads.insert(quads.end(), q, q + 4); }
            gpca_host::write_fstats(a.output_prefix, names, a.fstats_list, gpca::Engine::fstat(facc, fcnt, B, P, quads));
            std::snprintf(buf, sizeof buf, "%zu f-statistics over %zu SNPs in %d jackknife blocks (%s), written to %s.fstats", a.fstats_list.size(),
                          rows.size(), (int)B, a.fstat_block.c_str(), a.output_prefix.c_str());
            logmsg(buf);
        }
    }
    return 0;
}

const char* const kLdScoreNeedsResident =
    "error: --gpca-ld-score needs the genotype matrix resident on the device: with the matrix walked out of core a window crosses the "
    "panels, and the halo of rows that needs is not implemented\n";

// --gpca-ld-score WINDOW: the LD scores (gpca_ld_score, in the row bands of ld_next_band, always unbiased; the bands added up) of every
// SNP that passes the SNP QC, over every sample, into P.l2.ldscore, P.l2.M and P.l2.M_5_50.  Sets the keep mask to the QC mask (mu, sigma
// unchanged), which ends the fit's validity.  l2 receives L2 [K] (cli.py:_ld_score).
int run_ld_score(gpca::Engine& eng, const Args& a, const gpca_host::PlinkFileset& fs, const gpca::SnpStats& st, std::vector<double>& l2) {
    eng.set_standardization(st.mu, st.sigma, st.keep);                                // every SNP that passes the SNP QC
    std::vector<int64_t> rows, pos;
    std::vector<std::string> chrom, ids;
    for (size_t i = 0; i < st.keep.size(); ++i)
        if (st.keep[i]) { rows.push_back((int64_t)i); chrom.push_back(fs.chromosomes[i]); pos.push_back(fs.positions[i]); ids.push_back(fs.variant_ids[i]); }
    const int64_t K = (int64_t)rows.size();
    std::vector<int64_t> win_end;
    try { win_end = gpca_host::ld_windows(chrom, pos, a.ld_score); }
    catch (const std::runtime_error& e) {
        std::fprintf(stderr, "error: --gpca-ld-score: %s (variant indices count the SNPs that pass the SNP QC)\n", e.what());
        return 1;
    }
    std::vector<int64_t> acc((size_t)K, 0), part((size_t)K, 0);
    for (int64_t r0 = 0; r0 < K;) {
        int64_t r1 = 0, wm = 1;
        gpca_host::ld_next_band(win_end, r0, (int64_t)1 << 26, r1, wm);
        const std::vector<int64_t> we(win_end.begin() + r0, win_end.begin() + r1);
        std::vector<int64_t> score;
        std::vector<int32_t> partners;
        try { eng.ld_score(r0, r1, we, (int32_t)wm, true, score, &partners); }
        catch (const gpca::Error& e) {
            if (e.status() != GPCA_ERR_STATE) throw;
            std::fputs(kLdScoreNeedsResident, stderr);
            return 1;
        }
        gpca_host::ld_score_add_band(acc, part, r0, score, &partners);
        r0 = r1;
    }
    l2 = gpca::Engine::ld_score_total(acc);
    const std::vector<uint32_t> counts = eng.snp_qc_counts();
    std::vector<double> maf((size_t)K);
    for (size_t t = 0; t < (size_t)K; ++t) {
        const uint32_t* c = counts.data() + 4 * (size_t)rows[t];
        maf[t] = gpca_host::maf_from_counts(c[0], c[2], c[3]);
    }
    gpca_host::write_ldscore(a.output_prefix, chrom, ids, pos, l2, maf);
    double sum_l2 = 0.0;
    long long sum_p = 0;
    for (double v : l2) sum_l2 += v;
    for (int64_t v : part) sum_p += v;
    char buf[512];
    std::snprintf(buf, sizeof buf, "LD scores (window %s) of %lld SNPs over %lld samples: mean L2 %.6g, mean partners %.6g, written to %s.l2.ldscore",
                  a.ld_score.c_str(), (long long)K, (long long)eng.dims().second, K ? sum_l2 / (double)K : std::nan(""), K ? (double)sum_p / (double)K : std::nan(""),
                  a.output_prefix.c_str());
    logmsg(buf);
    return 0;
}

const char* const kAssocNeedsResident =
    "error: --gpca-assoc-pheno needs the genotype matrix resident on the device: the scan of a matrix walked out of core is not implemented\n";
constexpr int64_t kAssocMaxColumns = 64;

// --gpca-assoc-set-list FILE: the gene-level burden and SKAT tests (gpca_assoc_logistic_set, gpca_set_test) of every case / control
// trait, on the QC mask and the include set of the per-SNP scans, into P.<trait>.assoc.set; one row per set in file order
// (cli.py:_assoc_sets).  rows: the original row of every kept row; a1_freq: of every kept row; Yb [n][Tb].
void run_assoc_sets(gpca::Engine& eng, const Args& a, const gpca_host::PlinkFileset& fs, const std::vector<int64_t>& rows,
                    const std::vector<double>& a1_freq, const std::vector<double>& Yb, int32_t Tb, const std::vector<std::string>& bnames,
                    const std::vector<double>& C, int32_t Pc, const std::vector<uint8_t>& include) {
    const size_t n = include.size();
    std::vector<std::string> kept_ids;
    for (int64_t o : rows) kept_ids.push_back(fs.variant_ids[(size_t)o]);
    const std::vector<gpca_host::VariantSet> sets = gpca_host::read_set_list(a.assoc_set_list, kept_ids);
    const bool beta = a.assoc_set_weights == "beta";
    std::vector<std::vector<int64_t>> left(sets.size());
    std::vector<size_t> run;
    for (size_t i = 0; i < sets.size(); ++i) {
        for (int64_t r : sets[i].rows) if (gpca_host::set_maf_ok(a1_freq[(size_t)r], a.assoc_set_max_maf)) left[i].push_back(r);
        const int64_t m = (int64_t)left[i].size();
        if (m > gpca_host::kAssocSetMaxRows)
            std::fprintf(stderr, "note: --gpca-assoc-set-list: set %s keeps %lld variants, more than %lld: NA\n", sets[i].name.c_str(), (long long)m,
                         (long long)gpca_host::kAssocSetMaxRows);
        if (m >= 1 && m <= gpca_host::kAssocSetMaxRows) run.push_back(i);
    }
    std::vector<int64_t> sizes;
    for (size_t i : run) sizes.push_back((int64_t)left[i].size());
    // results [trait][set][10]; have [set]
    std::vector<std::vector<double>> results((size_t)Tb, std::vector<double>(sets.size() * 10, 0.0));
    std::vector<uint8_t> have(sets.size(), 0);
    for (const auto& g : gpca_host::assoc_score_groups(Tb, Pc)) {
        const int32_t Tg = (int32_t)(g.second - g.first);
        std::vector<double> Yg(n * (size_t)Tg);
        for (size_t s = 0; s < n; ++s)
            for (int32_t t = 0; t < Tg; ++t) Yg[s * (size_t)Tg + (size_t)t] = Yb[s * (size_t)Tb + (size_t)g.first + (size_t)t];
        for (const auto& c : gpca_host::assoc_set_groups(sizes, Tg, Pc)) {
            std::vector<int64_t> off(1, 0), list;
            for (int64_t k = c.first; k < c.second; ++k) {
                const std::vector<int64_t>& r = left[run[(size_t)k]];
                list.insert(list.end(), r.begin(), r.end());
                off.push_back((int64_t)list.size());
            }
            std::vector<double> stats, info, phi, ua;
            eng.assoc_logistic_set(Yg, Tg, C, Pc, &include, a.assoc_vif, off, list, stats, info, phi, &ua);
            size_t p0 = 0;
            for (int64_t k = c.first; k < c.second; ++k) {
                const size_t i = run[(size_t)k], lo = (size_t)off[(size_t)(k - c.first)], m = left[i].size(), tri = m * (m + 1) / 2;
                std::vector<double> u(m), w(m);
                for (size_t q = 0; q < m; ++q) w[q] = gpca_host::set_weight(info[5 * (lo + q) + 1], beta);
                for (int32_t t = 0; t < Tg; ++t) {
                    for (size_t q = 0; q < m; ++q)
                        u[q] = (info[5 * (lo + q) + 3] == 1.0 ? -1.0 : 1.0) * ua[((lo + q) * (size_t)Tg + (size_t)t) * (size_t)(Pc + 3)];
                    gpca::Engine::set_test(u, std::vector<double>(phi.begin() + (std::ptrdiff_t)(p0 + (size_t)t * tri), phi.begin() + (std::ptrdiff_t)(p0 + ((size_t)t + 1) * tri)),
                                           w, &results[(size_t)g.first + (size_t)t][i * 10]);
                }
                have[i] = 1;
                p0 += (size_t)Tg * tri;
            }
        }
    }
    for (int32_t t = 0; t < Tb; ++t) {
        gpca_host::AssocSetWriter w(a.output_prefix, bnames[(size_t)t]);
        for (size_t i = 0; i < sets.size(); ++i) w.add_row(sets[i], (int64_t)left[i].size(), have[i] ? &results[(size_t)t][i * 10] : nullptr);
    }
    char buf[512];
    std::snprintf(buf, sizeof buf, "set tests of %zu of %zu sets against %d case / control traits, written to %s.<trait>.assoc.set", run.size(), sets.size(),
                  (int)Tb, a.output_prefix.c_str());
    logmsg(buf);
}

const char* kQtlNeedsResident =
    "error: --gpca-qtl-pheno needs the genotype matrix resident on the device: the scan of a matrix walked out of core is not implemented\n";
constexpr int64_t kQtlMaxCovariates = 63, kQtlMaxTraits = (int64_t)1 << 20, kQtlCap = (int64_t)1 << 20;

// --gpca-qtl-cis-pos FILE: cis-QTL mapping (gpca_assoc_qtl_cis) of every trait of --gpca-qtl-pheno that FILE gives a position, against the
// SNPs that pass the SNP QC within --gpca-qtl-cis-window of it, with --gpca-qtl-cis-perm permutations from the table of
// --gpca-qtl-cis-seed, in bands of traits, into P.qtl.cis (cli.py:_qtl_cis).  Y [n][T], C [n][Pc], include, rows: run_qtl's.
int run_qtl_cis(gpca::Engine& eng, const Args& a, const gpca_host::PlinkFileset& fs, const std::vector<double>& Y, const std::vector<double>& C,
                int32_t Pc, const std::vector<uint8_t>& include, const std::vector<int64_t>& rows, int64_t n, int64_t n_inc, int64_t df) {
    const std::vector<std::string>& names = a.qtl_pheno_table.names;
    const int64_t T = (int64_t)names.size(), P = a.qtl_cis_perm;
    std::vector<std::string> chrom, tchrom((size_t)T);
    std::vector<int64_t> pos, tpos((size_t)T, 0);
    std::vector<uint8_t> have((size_t)T, 0);
    for (int64_t r : rows) { chrom.push_back(fs.chromosomes[(size_t)r]); pos.push_back(fs.positions[(size_t)r]); }
    int64_t n_pos = 0;
    for (int64_t t = 0; t < T; ++t) {
        const auto it = a.qtl_cis_table.find(names[(size_t)t]);
        if (it == a.qtl_cis_table.end()) continue;
        have[(size_t)t] = 1; tchrom[(size_t)t] = it->second.first; tpos[(size_t)t] = it->second.second; ++n_pos;
    }
    std::vector<int64_t> win;
    try { win = gpca_host::qtl_cis_windows(chrom, pos, tchrom, tpos, a.qtl_cis_window); }
    catch (const std::runtime_error& e) { std::fprintf(stderr, "error: --gpca-qtl-cis-pos: %s\n", e.what()); return 1; }
    for (int64_t t = 0; t < T; ++t) if (!have[(size_t)t]) win[2 * (size_t)t] = win[2 * (size_t)t + 1] = 0;
    std::vector<uint32_t> perm((size_t)P * (size_t)n_inc + 1);
    if (gpca_qtl_perm_table((uint64_t)a.qtl_cis_seed, n_inc, (int32_t)P, perm.data()) != GPCA_OK) {
        std::fprintf(stderr, "error: --gpca-qtl-cis-perm: the permutation table was refused\n");
        return 1;
    }
    std::vector<int64_t> n_var((size_t)T + 1), best_row((size_t)T + 1);
    std::vector<double> best_r2((size_t)T + 1), best_stat(3 * (size_t)T + 1), perm_r2((size_t)T * (size_t)P + 1);
    try {
        // (no SNP passes the SNP QC: nothing to ask the device; every trait with a position gets its N_VAR = 0 line)
        for (const auto& b : rows.empty() ? std::vector<std::pair<int64_t, int64_t>>() : gpca_host::assoc_qtl_cis_bands(T, P)) {
            const size_t g0 = (size_t)b.first, gn = (size_t)(b.second - b.first);
            std::vector<double> Yg((size_t)n * gn);
            for (int64_t s = 0; s < n; ++s)
                for (size_t j = 0; j < gn; ++j) Yg[(size_t)s * gn + j] = Y[(size_t)s * (size_t)T + g0 + j];
            eng.check(gpca_assoc_qtl_cis(eng.handle(), Yg.data(), (int64_t)gn, Pc ? C.data() : nullptr, Pc, include.data(), a.qtl_vif, &win[2 * g0],
                                         P ? perm.data() : nullptr, (int32_t)P, &n_var[g0], &best_row[g0], &best_r2[g0], &best_stat[3 * g0],
                                         P ? &perm_r2[g0 * (size_t)P] : nullptr));
        }
    } catch (const gpca::Error& e) {
        if (e.status() == GPCA_ERR_STATE) { std::fputs(kQtlNeedsResident, stderr); return 1; }
        throw;
    }
    gpca_host::ensure_parent(a.output_prefix);
    {
        gpca_host::QtlCisWriter w(a.output_prefix);
        const double nan = std::nan("");
        for (int64_t t = 0; t < T; ++t) {
            const size_t g = (size_t)t;
            if (!have[g]) { w.add_no_pos(names[g]); continue; }
            if (n_var[g] == 0) { w.add_empty(names[g], tchrom[g], tpos[g]); continue; }
            const size_t o = (size_t)rows[(size_t)best_row[g]];
            double v[9] = {nan, nan, nan, nan, nan, nan, nan, nan, nan};
            gpca_qtl_stats(best_stat[3 * g], best_stat[3 * g + 1], best_stat[3 * g + 2], (double)df, v);
            v[3] = v[2] != v[2] ? nan : gpca_student_t_log10p(v[2], (double)df);
            if (P > 0) {
                double ba[7];
                int32_t status = 0;
                gpca_qtl_beta_approx(&perm_r2[g * (size_t)P], P, best_r2[g], (double)df, ba, &status);
                v[4] = ba[1]; v[5] = ba[2]; v[6] = ba[3]; v[7] = ba[0]; v[8] = ba[5];
            }
            w.add_trait(names[g], tchrom[g], tpos[g], n_var[g], fs.variant_ids[o], fs.positions[o], fs.allele1[o], v);
        }
    }
    char buf[768];
    std::snprintf(buf, sizeof buf, "cis-QTL mapping of %lld of %lld traits within %lld bp with %d covariates on %lld of %lld samples and %lld permutations "
                  "(seed %lld), written to %s.qtl.cis", (long long)n_pos, (long long)T, (long long)a.qtl_cis_window, (int)Pc, (long long)n_inc, (long long)n,
                  (long long)P, (long long)a.qtl_cis_seed, a.output_prefix.c_str());
    logmsg(buf);
    return 0;
}

// The scan of every SNP against every trait of run_qtl, into P.qtl.hits and P.qtl.best (cli.py:_qtl_trans).  Y [n][T], C [n][Pc],
// include, rows (the SNPs that pass the SNP QC), df, r2_min and tmin are run_qtl's.
int run_qtl_trans(gpca::Engine& eng, const Args& a, const gpca_host::PlinkFileset& fs, const std::vector<double>& Y, const std::vector<double>& C,
                  int32_t Pc, int32_t P, const std::vector<uint8_t>& include, const std::vector<int64_t>& rows, int64_t T, int64_t n, int64_t n_inc,
                  int64_t df, double r2_min, double tmin) {
    const std::vector<std::string>& names = a.qtl_pheno_table.names;
    const double nan = std::nan("");
    std::vector<double> b2((size_t)T, nan), beta((size_t)T, nan), se((size_t)T, nan), tt((size_t)T, nan);
    std::vector<int64_t> bw((size_t)T, -1);
    int64_t n_tests = 0, n_hits = 0;
    auto log10p = [&](double t) { return t != t ? nan : gpca_student_t_log10p(t, (double)df); };
    try {
        {
            gpca_host::QtlHitsWriter w(a.output_prefix);
            for (const auto& b : gpca_host::assoc_qtl_bands((int64_t)rows.size(), T, n, kQtlCap)) {
                gpca::Engine::QtlResult q = eng.assoc_qtl(Y, T, C, Pc, &include, a.qtl_vif, r2_min, kQtlCap, b.first, b.second);
                if (q.n_found > kQtlCap) q = eng.assoc_qtl(Y, T, C, Pc, &include, a.qtl_vif, r2_min, q.n_found, b.first, b.second);   // once more
                for (int64_t r = b.first; r < b.second; ++r) {
                    const double* o = &q.rowinfo[4 * (size_t)(r - b.first)];
                    n_tests += !(o[0] == 0.0 || !(o[2] > 0.0) || o[3] * a.qtl_vif < o[2]);
                }
                for (int64_t i = 0; i < q.n_found; ++i) {
                    const size_t r = (size_t)q.rows[(size_t)i], t = (size_t)q.traits[(size_t)i], o = (size_t)rows[r];
                    const double* info = &q.rowinfo[4 * (r - (size_t)b.first)];
                    double s3[3];
                    gpca_qtl_stats(q.xb[(size_t)i], info[3], q.yy[t], (double)df, s3);
                    w.add_hit(fs.chromosomes[o], fs.positions[o], fs.variant_ids[o], fs.allele1[o], names[t], info[0], info[1], s3[0], s3[1], s3[2], log10p(s3[2]));
                }
                n_hits += q.n_found;
                gpca_host::qtl_best_merge(b2, bw, q.best_r2, q.best_row);
            }
        }
        // the best SNP of every trait: gpca_assoc_linear on that SNP, the traits that share a SNP in groups of 64 - Pc
        std::map<int64_t, std::vector<int64_t>> by_row;
        for (int64_t t = 0; t < T; ++t) if (bw[(size_t)t] >= 0) by_row[bw[(size_t)t]].push_back(t);
        const int64_t gmax = 64 - Pc;
        for (const auto& kv : by_row)
            for (size_t g0 = 0; g0 < kv.second.size(); g0 += (size_t)gmax) {
                const size_t gn = std::min<size_t>((size_t)gmax, kv.second.size() - g0);
                std::vector<double> Yg((size_t)n * gn), stats, info;
                for (int64_t s = 0; s < n; ++s)
                    for (size_t j = 0; j < gn; ++j) Yg[(size_t)s * gn + j] = Y[(size_t)s * (size_t)T + (size_t)kv.second[g0 + j]];
                eng.assoc_linear(Yg, (int32_t)gn, C, Pc, &include, a.qtl_vif, kv.first, kv.first + 1, stats, info);
                for (size_t j = 0; j < gn; ++j) {
                    const size_t t = (size_t)kv.second[g0 + j];
                    beta[t] = stats[3 * j]; se[t] = stats[3 * j + 1]; tt[t] = stats[3 * j + 2];
                }
            }
    } catch (const gpca::Error& e) {
        if (e.status() == GPCA_ERR_STATE) { std::fputs(kQtlNeedsResident, stderr); return 1; }
        throw;
    }
    {
        gpca_host::QtlBestWriter w(a.output_prefix);
        for (int64_t t = 0; t < T; ++t) {
            if (bw[(size_t)t] < 0) { w.add_none(names[(size_t)t], 0); continue; }
            const size_t o = (size_t)rows[(size_t)bw[(size_t)t]];
            w.add_trait(names[(size_t)t], fs.chromosomes[o], fs.positions[o], fs.variant_ids[o], fs.allele1[o], beta[(size_t)t], se[(size_t)t], tt[(size_t)t],
                        log10p(tt[(size_t)t]), n_tests);
        }
    }
    char buf[768];
    std::snprintf(buf, sizeof buf, "QTL scan of %zu SNPs against %lld traits with %d covariates (%d PCs) on %lld of %lld samples: %lld pairs with |t| >= %.6g, "
                  "written to %s.qtl.hits and %s.qtl.best", rows.size(), (long long)T, (int)Pc, (int)P, (long long)n_inc, (long long)n, (long long)n_hits, tmin,
                  a.output_prefix.c_str(), a.output_prefix.c_str());
    logmsg(buf);
    return 0;
}

// --gpca-qtl-pheno FILE: the many-trait QTL scan (gpca_assoc_qtl) of every SNP that passes the SNP QC against every column of FILE, in
// row bands, into P.qtl.hits and P.qtl.best.  Runs last, after the association scan: it resets the keep mask to the QC mask.  Covariates
// and the include rule are the association scan's; the statistics of a hit come from gpca_qtl_stats, those of a trait's best SNP from
// gpca_assoc_linear on that SNP (cli.py:_qtl).  scores is [n][kc].
int run_qtl(gpca::Engine& eng, const Args& a, const gpca_host::PlinkFileset& fs, const std::vector<std::string>& fids,
            const std::vector<std::string>& sample_ids, const std::vector<double>& scores, int kc, const std::vector<uint8_t>& inset,
            const gpca::SnpStats& st) {
    const int64_t n = (int64_t)sample_ids.size();
    const int32_t P = a.have_qtl_pcs ? (int32_t)a.qtl_pcs : (int32_t)kc;
    const int64_t T = (int64_t)a.qtl_pheno_table.names.size();
    const int32_t nc = a.qtl_covar.empty() ? 0 : (int32_t)a.qtl_covar_table.names.size();
    const int32_t Pc = P + nc;
    const std::vector<double> Y = gpca_host::align_pheno(a.qtl_pheno_table, fids, sample_ids);
    std::vector<double> cv;
    if (nc) cv = gpca_host::align_pheno(a.qtl_covar_table, fids, sample_ids);
    std::vector<double> C((size_t)n * (size_t)Pc + 1);
    std::vector<uint8_t> include((size_t)n, 1);
    int64_t n_inc = 0;
    for (int64_t s = 0; s < n; ++s) {
        bool ok = inset.empty() || inset[(size_t)s];
        for (int32_t c = 0; c < P; ++c) C[(size_t)s * Pc + c] = scores[(size_t)s * kc + c];
        for (int32_t c = 0; c < nc; ++c) C[(size_t)s * Pc + P + c] = cv[(size_t)s * nc + c];
        for (int32_t c = 0; c < Pc; ++c) ok = ok && std::isfinite(C[(size_t)s * Pc + c]);
        for (int64_t t = 0; t < T; ++t) ok = ok && std::isfinite(Y[(size_t)s * (size_t)T + (size_t)t]);
        include[(size_t)s] = ok ? 1 : 0;
        n_inc += ok;
    }
    const int64_t df = n_inc - Pc - 2;
    if (df < 1) {
        std::fprintf(stderr, "error: --gpca-qtl-pheno: %lld samples have every trait and covariate, which leaves no degree of freedom beside %d covariates\n",
                     (long long)n_inc, (int)Pc);
        return 1;
    }
    const double tmin = a.have_qtl_t ? a.qtl_t : gpca_qtl_t_min(a.qtl_log10p, (double)df);
    if (!(tmin < INFINITY)) {
        std::fprintf(stderr, "error: --gpca-qtl-log10p: no finite t reaches the threshold at %lld degrees of freedom\n", (long long)df);
        return 1;
    }
    const double r2_min = tmin * tmin / (tmin * tmin + (double)df);
    eng.set_standardization(st.mu, st.sigma, st.keep);                                // every SNP that passes the SNP QC
    std::vector<int64_t> rows;
    for (size_t i = 0; i < st.keep.size(); ++i) if (st.keep[i]) rows.push_back((int64_t)i);
    gpca_host::ensure_parent(a.output_prefix);
    if (!a.qtl_cis_only) {
        const int rc = run_qtl_trans(eng, a, fs, Y, C, Pc, P, include, rows, T, n, n_inc, df, r2_min, tmin);
        if (rc) return rc;
    }
    if (!a.qtl_cis_pos.empty()) return run_qtl_cis(eng, a, fs, Y, C, Pc, include, rows, n, n_inc, df);
    return 0;
}

// --gpca-assoc-pheno FILE: the linear association scan (gpca_assoc_linear) of every SNP that passes the SNP QC, in row bands, into
// P.<trait>.assoc.linear.  Runs last: it resets the keep mask to the QC mask (mu, sigma unchanged), which ends the fit's validity.
// Covariates = the first P columns of the scores the run wrote, then the columns of --gpca-assoc-covar; a sample is included when every
// trait and covariate is present for it and it is in the KING in-set, when there is one (cli.py:_assoc).  scores is [n][kc].
int run_assoc(gpca::Engine& eng, const Args& a, const gpca_host::PlinkFileset& fs, const std::vector<std::string>& fids,
              const std::vector<std::string>& sample_ids, const std::vector<double>& scores, int kc, const std::vector<uint8_t>& inset,
              const gpca::SnpStats& st, const std::vector<double>& l2) {
    const int64_t n = (int64_t)sample_ids.size();
    const int32_t P = a.have_assoc_pcs ? (int32_t)a.assoc_pcs : (int32_t)kc;
    const int32_t T = (int32_t)a.assoc_pheno_table.names.size(), nc = a.assoc_covar.empty() ? 0 : (int32_t)a.assoc_covar_table.names.size();
    const int32_t Pc = P + nc;
    const std::vector<double> Y = gpca_host::align_pheno(a.assoc_pheno_table, fids, sample_ids);
    std::vector<double> cv;
    if (nc) cv = gpca_host::align_pheno(a.assoc_covar_table, fids, sample_ids);
    std::vector<double> C((size_t)n * (size_t)Pc + 1);
    std::vector<uint8_t> include((size_t)n, 1);
    int64_t n_inc = 0;
    for (int64_t s = 0; s < n; ++s) {
        bool ok = inset.empty() || inset[(size_t)s];
        for (int32_t c = 0; c < P; ++c) C[(size_t)s * Pc + c] = scores[(size_t)s * kc + c];
        for (int32_t c = 0; c < nc; ++c) C[(size_t)s * Pc + P + c] = cv[(size_t)s * nc + c];
        for (int32_t c = 0; c < Pc; ++c) ok = ok && std::isfinite(C[(size_t)s * Pc + c]);
        for (int32_t t = 0; t < T; ++t) ok = ok && std::isfinite(Y[(size_t)s * T + t]);
        include[(size_t)s] = ok ? 1 : 0;
        n_inc += ok;
    }
    const int64_t df = n_inc - Pc - 2;
    if (df < 1) {
        std::fprintf(stderr, "error: --gpca-assoc-pheno: %lld samples have every trait and covariate, which leaves no degree of freedom beside %d covariates\n",
                     (long long)n_inc, (int)Pc);
        return 1;
    }
    // --gpca-assoc-logistic: the binary columns (recoded to 0 / 1) leave the linear scan for the score scan
    const int32_t Tall = T;
    std::vector<std::string> names = a.assoc_pheno_table.names, bnames;
    std::vector<double> Yq = Y, Yb;
    int32_t Tq = Tall, Tb = 0;
    if (a.assoc_logistic) {
        std::vector<int32_t> qcols, bcols;
        std::vector<double> shift;
        for (int32_t j = 0; j < Tall; ++j) {
            double sh = 0.0;
            if (gpca_host::binary_trait(a.assoc_pheno_table, (size_t)j, &sh)) { bcols.push_back(j); shift.push_back(sh); } else qcols.push_back(j);
        }
        Tq = (int32_t)qcols.size(); Tb = (int32_t)bcols.size();
        names.clear();
        for (int32_t j : qcols) names.push_back(a.assoc_pheno_table.names[(size_t)j]);
        for (int32_t j : bcols) bnames.push_back(a.assoc_pheno_table.names[(size_t)j]);
        Yq.assign((size_t)n * (size_t)Tq + 1, 0.0); Yb.assign((size_t)n * (size_t)Tb + 1, 0.0);
        for (int64_t s = 0; s < n; ++s) {
            for (int32_t j = 0; j < Tq; ++j) Yq[(size_t)s * Tq + j] = Y[(size_t)s * Tall + qcols[(size_t)j]];
            for (int32_t j = 0; j < Tb; ++j) Yb[(size_t)s * Tb + j] = include[(size_t)s] ? Y[(size_t)s * Tall + bcols[(size_t)j]] - shift[(size_t)j] : 0.0;
        }
        for (int32_t j = 0; j < Tb; ++j) {                                            // before any file of the trait is written
            std::vector<double> y((size_t)n), alpha, mu;
            for (int64_t s = 0; s < n; ++s) y[(size_t)s] = Yb[(size_t)s * Tb + j];
            try { gpca::Engine::logistic_null(y, C, Pc, &include, alpha, mu); }
            catch (const gpca::Error& e) {
                // (cli.py:LOGISTIC_NULL_FAILURES)
                const char* why = e.status() == GPCA_ERR_BAD_ARG ? "the included samples hold one class only, or a covariate is constant or collinear over them"
                                  : e.status() == GPCA_ERR_NOT_CONVERGED ? "Newton's method does not converge: the covariates separate the cases from the controls"
                                                                         : gpca_status_string(e.status());
                std::fprintf(stderr, "error: --gpca-assoc-logistic: trait %s: the null model cannot be fitted (%s)\n", bnames[(size_t)j].c_str(), why);
                return 1;
            }
        }
    }
    eng.set_standardization(st.mu, st.sigma, st.keep);                                // every SNP that passes the SNP QC
    std::vector<int64_t> rows;
    for (size_t i = 0; i < st.keep.size(); ++i) if (st.keep[i]) rows.push_back((int64_t)i);
    gpca_host::ensure_parent(a.output_prefix);
    std::vector<double> a1_all(rows.size(), std::nan(""));                            // (of every kept row, for the sets' MAF rule)
    // --gpca-assoc-ldsc: chi2 of every trait over the rows (NaN where there is no statistic), the quantitative traits first
    std::vector<std::vector<double>> chi2q, chi2b;
    if (a.assoc_ldsc) { chi2q.assign((size_t)Tq, std::vector<double>(rows.size(), std::nan(""))); chi2b.assign((size_t)Tb, std::vector<double>(rows.size(), std::nan(""))); }
    try {
        if (a.assoc_cc_freq && Tb) {
            // --gpca-assoc-cc-freq: the counts among the controls and the cases of every case / control trait, over the scan's include
            // set (label -1 outside it), into P.<trait>.frq.cc (cli.py:_cc_freq)
            for (int32_t t = 0; t < Tb; ++t) {
                std::vector<int32_t> labels((size_t)n);
                for (int64_t s = 0; s < n; ++s) labels[(size_t)s] = include[(size_t)s] ? (int32_t)Yb[(size_t)s * Tb + t] : -1;
                gpca_host::FrqStratWriter w(a.output_prefix + "." + bnames[(size_t)t] + ".frq.cc", {"CTRL", "CASE"}, gpca_hwe_chi_squared_p_value);
                for (const auto& b : gpca_host::group_count_bands((int64_t)rows.size(), 2)) {
                    std::vector<uint32_t> c;
                    eng.group_counts(labels, 2, b.first, b.second, c);
                    for (int64_t r = b.first; r < b.second; ++r) {
                        const size_t o = (size_t)rows[(size_t)r];
                        w.add_row(fs.chromosomes[o], fs.positions[o], fs.variant_ids[o], fs.allele1[o], &c[(size_t)(r - b.first) * 6]);
                    }
                }
            }
            char cb[512];
            std::snprintf(cb, sizeof cb, "case / control genotype counts of %zu SNPs for %d traits, written to %s.<trait>.frq.cc", rows.size(), (int)Tb,
                          a.output_prefix.c_str());
            logmsg(cb);
        }
        if (Tq) {
            std::vector<std::unique_ptr<gpca_host::AssocWriter>> w;
            for (int32_t t = 0; t < Tq; ++t) w.emplace_back(new gpca_host::AssocWriter(a.output_prefix, names[(size_t)t]));
            for (const auto& b : gpca_host::assoc_bands((int64_t)rows.size(), Tq + Pc)) {
                std::vector<double> stats, info;
                eng.assoc_linear(Yq, Tq, C, Pc, &include, a.assoc_vif, b.first, b.second, stats, info);
                for (int64_t r = b.first; r < b.second; ++r) {
                    const size_t i = (size_t)(r - b.first), o = (size_t)rows[(size_t)r];
                    for (int32_t t = 0; t < Tq; ++t) {
                        const double* s3 = &stats[(i * (size_t)Tq + (size_t)t) * 3];
                        const double lp = s3[2] != s3[2] ? std::nan("") : gpca_student_t_log10p(s3[2], (double)df);
                        w[(size_t)t]->add_row(fs.chromosomes[o], fs.positions[o], fs.variant_ids[o], fs.allele1[o], info[4 * i], info[4 * i + 1], s3[0], s3[1], s3[2], lp);
                        if (a.assoc_ldsc) chi2q[(size_t)t][(size_t)r] = s3[2] * s3[2];
                    }
                }
            }
        }
        if (Tb) {
            for (const auto& g : gpca_host::assoc_score_groups(Tb, Pc)) {
                const int32_t Tg = (int32_t)(g.second - g.first);
                std::vector<double> Yg((size_t)n * (size_t)Tg);
                for (int64_t s = 0; s < n; ++s)
                    for (int32_t t = 0; t < Tg; ++t) Yg[(size_t)s * Tg + t] = Yb[(size_t)s * Tb + (size_t)g.first + t];
                std::vector<std::unique_ptr<gpca_host::AssocLogisticWriter>> w;
                for (int32_t t = 0; t < Tg; ++t) w.emplace_back(new gpca_host::AssocLogisticWriter(a.output_prefix, bnames[(size_t)g.first + t], a.assoc_spa, a.assoc_firth));
                for (const auto& b : gpca_host::assoc_score_bands((int64_t)rows.size(), Tg, Pc)) {
                    std::vector<double> stats, info, spa, firth;
                    if (a.assoc_firth) eng.assoc_logistic_firth(Yg, Tg, C, Pc, &include, a.assoc_vif, a.assoc_firth_z, b.first, b.second, stats, firth, info);
                    else if (a.assoc_spa) eng.assoc_logistic_spa(Yg, Tg, C, Pc, &include, a.assoc_vif, a.assoc_spa_z, b.first, b.second, stats, spa, info);
                    else eng.assoc_logistic_score(Yg, Tg, C, Pc, &include, a.assoc_vif, b.first, b.second, stats, info);
                    for (int64_t r = b.first; r < b.second; ++r) {
                        const size_t i = (size_t)(r - b.first), o = (size_t)rows[(size_t)r];
                        a1_all[(size_t)r] = info[5 * i + 1];
                        for (int32_t t = 0; t < Tg; ++t) {
                            const double* s5 = &stats[(i * (size_t)Tg + (size_t)t) * 5];
                            const double* s4 = a.assoc_spa ? &spa[(i * (size_t)Tg + (size_t)t) * 4] : nullptr;
                            const double* f5 = a.assoc_firth ? &firth[(i * (size_t)Tg + (size_t)t) * 5] : nullptr;
                            const double lp = f5 ? f5[0] : (s4 ? s4[0] : (s5[2] != s5[2] ? std::nan("") : gpca_normal_log10p(s5[2])));
                            const bool fy = f5 && f5[1] == 1.0;                     // (corrected: BETA and SE are Firth's)
                            w[(size_t)t]->add_row(fs.chromosomes[o], fs.positions[o], fs.variant_ids[o], fs.allele1[o], info[5 * i], info[5 * i + 1],
                                                  fy ? f5[2] : s5[0], fy ? f5[3] : s5[1], s5[2], lp, f5 ? (int)f5[1] : (s4 ? (int)s4[1] : 0));
                            if (a.assoc_ldsc) chi2b[(size_t)g.first + (size_t)t][(size_t)r] = s5[2] * s5[2];
                        }
                    }
                }
            }
        }
        if (Tb && !a.assoc_set_list.empty()) run_assoc_sets(eng, a, fs, rows, a1_all, Yb, Tb, bnames, C, Pc, include);
    } catch (const gpca::Error& e) {
        if (e.status() != GPCA_ERR_STATE) throw;
        std::fputs(kAssocNeedsResident, stderr);
        return 1;
    }
    char buf[512];
    std::snprintf(buf, sizeof buf, "association scan of %zu SNPs against %d traits with %d covariates (%d PCs) on %lld of %lld samples, written to %s.<trait>.assoc.linear",
                  rows.size(), (int)Tq, (int)Pc, (int)P, (long long)n_inc, (long long)n, a.output_prefix.c_str());
    logmsg(buf);
    if (Tb) {
        std::snprintf(buf, sizeof buf, "logistic score scan of %zu SNPs against %d case / control traits with %d covariates on %lld of %lld samples, written to %s.<trait>.assoc.logistic",
                      rows.size(), (int)Tb, (int)Pc, (long long)n_inc, (long long)n, a.output_prefix.c_str());
        logmsg(buf);
    }
    if (a.assoc_ldsc) {
        // one LD-score regression per trait in file order; chi2 = T_STAT^2 or the score Z_STAT^2, NaN rows drop out (cli.py:_assoc)
        std::vector<gpca_host::LdscRow> out;
        for (const std::string& name : a.assoc_pheno_table.names) {
            const auto qb = std::find(bnames.begin(), bnames.end(), name);
            const bool bin = qb != bnames.end();
            const std::vector<double>& c2 = bin ? chi2b[(size_t)(qb - bnames.begin())] : chi2q[(size_t)(std::find(names.begin(), names.end(), name) - names.begin())];
            gpca_host::LdscRow row{name, bin ? "LOGISTIC" : "LINEAR", n_inc, {}};
            try { row.fit = gpca::Engine::ldsc_fit(c2, l2, (double)n_inc, (double)rows.size(), nullptr, 200, std::max(0.001 * (double)n_inc, 80.0)); }
            catch (const gpca::Error&) {
                std::fprintf(stderr, "note: --gpca-assoc-ldsc: trait %s: too few SNPs with a statistic, or LD scores without spread: NA\n", name.c_str());
            }
            out.push_back(row);
        }
        gpca_host::write_ldsc_summary(a.output_prefix, out);
        std::snprintf(buf, sizeof buf, "LD-score regression of %zu traits over %zu SNPs, written to %s.ldsc.summary", out.size(), rows.size(), a.output_prefix.c_str());
        logmsg(buf);
    }
    return 0;
}

const char* const kSampleQcNeedsResident =
    "error: --gpca-sample-missing, --gpca-het, --gpca-mind and --gpca-het-sd need the genotype matrix resident on the device: the "
    "per-sample counts of a matrix walked out of core are not implemented\n";

// --gpca-sample-missing / --gpca-het / --gpca-mind / --gpca-het-sd: the per-sample counts (gpca_sample_counts, in row bands) over every
// SNP that passes the SNP QC, with the rows' weights from the QC counts of all samples (gpca_het_weights), into P.smiss and P.het; with
// a filter, the pass mask and P.sampleqc.in.id / .out.id.  Sets the keep mask to the QC mask (mu, sigma unchanged); the caller sets its
// own afterwards.  pass stays empty without a filter (cli.py:_sample_qc).
int run_sample_qc(gpca::Engine& eng, const Args& a, const std::vector<std::string>& fids, const std::vector<std::string>& sample_ids,
                  const gpca::SnpStats& st, std::vector<uint8_t>& pass) {
    const size_t n = sample_ids.size();
    eng.set_standardization(st.mu, st.sigma, st.keep);                                 // every SNP that passes the SNP QC
    std::vector<int64_t> rows;
    for (size_t i = 0; i < st.keep.size(); ++i) if (st.keep[i]) rows.push_back((int64_t)i);
    const int64_t K = (int64_t)rows.size();
    const bool need_het = a.het || a.have_het_sd;
    std::vector<uint32_t> q;
    if (need_het) {
        const std::vector<uint32_t> all = eng.snp_qc_counts();
        std::vector<uint32_t> qc(4 * rows.size());
        for (size_t t = 0; t < rows.size(); ++t) std::copy(all.begin() + 4 * rows[t], all.begin() + 4 * rows[t] + 4, qc.begin() + 4 * t);
        q = gpca::Engine::het_weights(qc);
    }
    std::vector<uint32_t> counts(3 * n, 0u);
    std::vector<uint64_t> qsum(n, 0u);
    try {
        for (const auto& b : gpca_host::sample_count_bands(K)) {
            std::vector<uint32_t> c;
            std::vector<uint64_t> s;
            const std::vector<uint32_t> qb(need_het ? q.begin() + b.first : q.begin(), need_het ? q.begin() + b.second : q.begin());
            eng.sample_counts(b.first, b.second, need_het ? &qb : nullptr, c, need_het ? &s : nullptr);
            for (size_t i = 0; i < 3 * n; ++i) counts[i] += c[i];
            if (need_het) for (size_t i = 0; i < n; ++i) qsum[i] += s[i];
        }
    } catch (const gpca::Error& e) {
        if (e.status() != GPCA_ERR_STATE) throw;
        std::fputs(kSampleQcNeedsResident, stderr);
        return 1;
    }
    std::vector<double> het, F;
    if (need_het) {
        het = gpca::Engine::sample_het(counts, qsum);
        F.resize(n);
        for (size_t i = 0; i < n; ++i) F[i] = het[3 * i + 2];
    }
    gpca_host::ensure_parent(a.output_prefix);
    char buf[320];
    if (a.sample_missing) {
        gpca_host::write_smiss(a.output_prefix, fids, sample_ids, counts, K);
        std::snprintf(buf, sizeof buf, "missing calls of %zu samples over %lld SNPs written to %s.smiss", n, (long long)K, a.output_prefix.c_str());
        logmsg(buf);
    }
    if (a.het) {
        gpca_host::write_het(a.output_prefix, fids, sample_ids, counts, het);
        std::snprintf(buf, sizeof buf, "heterozygosity of %zu samples over %lld SNPs written to %s.het", n, (long long)K, a.output_prefix.c_str());
        logmsg(buf);
    }
    if (!a.have_mind && !a.have_het_sd) return 0;
    std::vector<uint8_t> reason;
    gpca_host::sample_qc_pass(counts, K, F, a.have_mind, a.mind, a.have_het_sd, a.het_sd, pass, reason);
    gpca_host::write_sample_qc_ids(a.output_prefix, fids, sample_ids, pass, reason);
    int64_t n_mind = 0, n_het = 0, n_ok = 0;
    for (size_t i = 0; i < n; ++i) { n_mind += reason[i] == gpca_host::kSampleQcMind; n_het += reason[i] == gpca_host::kSampleQcHet; n_ok += pass[i]; }
    std::snprintf(buf, sizeof buf, "sample QC: %lld samples fail --gpca-mind, %lld fail --gpca-het-sd, %lld of %zu pass", (long long)n_mind, (long long)n_het,
                  (long long)n_ok, n);
    logmsg(buf);
    return 0;
}

const char* const kHomozygNeedsResident =
    "error: --gpca-homozyg needs the genotype matrix resident on the device: the runs of homozygosity of a matrix walked out of core are "
    "not implemented\n";

// kb on the command line -> bp: x 1000 rounded half up (cli.py: math.floor(x * 1000.0 + 0.5))
inline int64_t kb_to_bp(double kb) { return (int64_t)std::floor(kb * 1000.0 + 0.5); }

const char* const kAdmixNeedsResident =
    "error: --gpca-admixture needs the genotype matrix resident on the device: the fit of a matrix walked out of core is not implemented\n";

// --gpca-admixture K: the admixture fit (gpca_admix) over the rows the PCA was fitted on (the handle's keep mask as the PCA left it) and
// every sample: mode 0 inside the in-set, mode 2 outside it, mode 1 for a sample with a group under --gpca-admixture-supervised; writes
// P.K.Q, .Q.id, .P, .P.id and .admix.log with the columns in admix_order (cli.py:_admix).
int run_admix(gpca::Engine& eng, const Args& a, const std::vector<std::string>& fids, const std::vector<std::string>& sample_ids,
              const std::vector<std::string>& vids, const std::vector<uint8_t>& inset) {
    const int K = (int)a.admix_k;
    const size_t n = sample_ids.size();
    std::vector<uint8_t> mode(n, 0);
    if (!inset.empty()) for (size_t s = 0; s < n; ++s) mode[s] = inset[s] ? 0 : 2;
    gpca_admix_params par{};
    par.K = K; par.max_iter = (int32_t)a.admix_max_iter; par.seed = (uint64_t)a.admix_seed; par.tol = a.admix_tol; par.accel = a.admix_no_accel ? 0 : 1;
    std::vector<float> Q, F, Q0, F0;
    gpca_admix_info info{};
    try {
        if (a.admix_supervised) {
            const std::vector<int32_t> labels = gpca_host::align_within(a.within_table, fids, sample_ids);
            eng.admix_init(K, par.seed, Q, F);
            const std::vector<uint8_t> fixed = gpca_host::admix_supervised(labels, K, Q);
            for (size_t s = 0; s < n; ++s) if (fixed[s]) mode[s] = 1;                     // a labelled sample is a reference wherever it stands
            par.init = 1;
            if (a.admix_cv) { Q0 = Q; F0 = F; }                                           // the cross-validation starts every fold from here
        }
        info = eng.admix(par, &mode, Q, F);
    } catch (const gpca::Error& e) {
        if (e.status() != GPCA_ERR_STATE) throw;
        std::fputs(kAdmixNeedsResident, stderr);
        return 1;
    }
    const std::vector<int64_t> order = gpca_host::admix_order(Q, n, K, mode);
    gpca_host::ensure_parent(a.output_prefix);
    gpca_host::write_admix(a.output_prefix, K, fids, sample_ids, vids, Q, F, order, par.seed, info.steps, info.cycles, info.converged != 0, info.loglik);
    char buf[512];
    std::snprintf(buf, sizeof buf, "admixture (K = %d) of %zu samples (%lld references, %lld projected) over %zu SNPs: %lld steps, %s, log-likelihood %.4f, written to %s.%d.Q",
                  K, n, (long long)std::count(mode.begin(), mode.end(), (uint8_t)1), (long long)std::count(mode.begin(), mode.end(), (uint8_t)2), vids.size(),
                  (long long)info.steps, info.converged ? "converged" : "not converged", info.loglik, a.output_prefix.c_str(), K);
    logmsg(buf);
    if (a.admix_cv) {
        // --gpca-admixture-cv: the same mode bytes, seed, max-iter, tol and accel, and the supervised fit's start; every K of the range
        std::vector<gpca_host::AdmixCvRow> table;
        std::string ks;
        for (int k : a.admix_cv_ks) {
            gpca_admix_params cp = par;
            cp.K = k;
            std::vector<gpca_admix_cv_fold_info> fo;
            const double cv = eng.admix_cv(cp, &mode, (int32_t)a.admix_cv_folds, (uint64_t)a.admix_cv_seed, &Q0, &F0, fo);
            for (size_t c = 0; c < fo.size(); ++c)
                table.push_back(gpca_host::AdmixCvRow{k, (int)a.admix_cv_folds, (uint64_t)a.admix_cv_seed, (int)c, fo[c].steps, fo[c].converged != 0, fo[c].n_held, fo[c].deviance});
            if (cv != cv) std::snprintf(buf, sizeof buf, "CV error (K=%d): NA", k);
            else std::snprintf(buf, sizeof buf, "CV error (K=%d): %.6f", k, cv);
            logmsg(buf);
            ks += (ks.empty() ? "" : ", ") + std::to_string(k);
        }
        gpca_host::write_admix_cv(a.output_prefix, table);
        std::snprintf(buf, sizeof buf, "admixture cross-validation (%lld folds, seed %lld) of K = %s written to %s.admix.cv", (long long)a.admix_cv_folds,
                      (long long)a.admix_cv_seed, ks.c_str(), a.output_prefix.c_str());
        logmsg(buf);
    }
    return 0;
}

// --gpca-homozyg: the runs of homozygosity (gpca_roh, in bands cut at chromosome starts) of every sample over every SNP that passes the
// SNP QC, the length and density rule on the records (gpca_roh_select), P.hom and P.hom.indiv.  Sets the keep mask to the QC mask (mu,
// sigma unchanged); the caller sets its own afterwards (cli.py:_homozyg).
int run_homozyg(gpca::Engine& eng, const Args& a, const gpca_host::PlinkFileset& fs, const std::vector<std::string>& fids,
                const std::vector<std::string>& sample_ids, const gpca::SnpStats& st) {
    eng.set_standardization(st.mu, st.sigma, st.keep);                                 // every SNP that passes the SNP QC
    std::vector<std::string> chroms, ids;
    std::vector<int64_t> pos;
    for (size_t i = 0; i < st.keep.size(); ++i)
        if (st.keep[i]) { chroms.push_back(fs.chromosomes[i]); ids.push_back(fs.variant_ids[i]); pos.push_back(fs.positions[i]); }
    const std::vector<uint8_t> brk = gpca_host::roh_breaks(chroms, pos, kb_to_bp(a.hom_gap));
    gpca_roh_params par{};
    par.window_snp = (int32_t)a.hom_window_snp; par.window_het = (int32_t)a.hom_window_het; par.window_missing = (int32_t)a.hom_window_missing;
    par.thr_num = (int32_t)a.hom_thr_num; par.thr_den = (int32_t)a.hom_thr_den; par.min_snp = (int32_t)a.hom_snp;
    par.max_het = a.have_hom_het ? (int32_t)a.hom_het : -1;
    std::vector<uint32_t> segs;                                                        // bands in row order: ordered by sample below
    try {
        for (const auto& b : gpca_host::roh_bands(brk)) {
            std::vector<uint32_t> s, c;
            eng.roh(b.first, b.second, std::vector<uint8_t>(brk.begin() + b.first, brk.begin() + b.second), par, s, c);
            segs.insert(segs.end(), s.begin(), s.end());
        }
    } catch (const gpca::Error& e) {
        if (e.status() != GPCA_ERR_STATE) throw;
        std::fputs(kHomozygNeedsResident, stderr);
        return 1;
    }
    // ascending (sample, first): the bands are disjoint in rows, so a stable sort by sample keeps the positions in order
    const size_t nrec = segs.size() / 5;
    std::vector<size_t> order(nrec);
    for (size_t i = 0; i < nrec; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return segs[5 * x] < segs[5 * y]; });
    std::vector<uint32_t> sorted(segs.size());
    for (size_t i = 0; i < nrec; ++i) std::copy(segs.begin() + 5 * order[i], segs.begin() + 5 * order[i] + 5, sorted.begin() + 5 * i);
    const std::vector<uint8_t> keep = gpca::Engine::roh_select(sorted, pos, kb_to_bp(a.hom_kb), kb_to_bp(a.hom_density));
    gpca_host::ensure_parent(a.output_prefix);
    gpca_host::write_hom(a.output_prefix, fids, sample_ids, chroms, ids, pos, sorted, keep, brk);
    char buf[384];
    std::snprintf(buf, sizeof buf, "runs of homozygosity of %zu samples over %zu SNPs: %lld of %zu runs pass the length and density rule, written to %s.hom",
                  sample_ids.size(), pos.size(), (long long)std::count(keep.begin(), keep.end(), (uint8_t)1), nrec, a.output_prefix.c_str());
    logmsg(buf);
    return 0;
}

int run_eigensnp_workflow(Args a) {
    if (a.bed_file.empty() || a.ld_block_file.empty()) {
        std::fprintf(stderr, "error: --bed-file and --ld-block-file are required when --eigensnp is used\n");           // main.rs:296-301
        return 2;
    }
    const auto t0 = std::chrono::steady_clock::now();
    gpca_host::PlinkFileset fs;
    gpca_host::read_plink(a.bed_file, fs);
    const int store = engine_storage(a, fs.n_samples);
    gpca::Engine eng(a.device, engine_precision(a), store);
    std::vector<std::string> sample_ids = fs.sample_ids;
    KeptColumns kept{&fs, {}};
    bool use_kept = false;
    if (!a.sample_keep_file.empty()) {                                                                                  // prepare.rs:1058-1096
        const auto ids = gpca_host::read_sample_keep_file(a.sample_keep_file);
        const std::set<std::string> keep_ids(ids.begin(), ids.end());
        sample_ids.clear();
        for (size_t i = 0; i < fs.sample_ids.size(); ++i)
            if (keep_ids.count(fs.sample_ids[i])) { kept.cols.push_back((int64_t)i); sample_ids.push_back(fs.sample_ids[i]); }
        if (kept.cols.empty()) { logmsg("No samples available after sample QC."); return 0; }
        use_kept = true;
    }
    const bool streamed = load_bed(eng, a, fs, use_kept ? &kept : nullptr);
    if (streamed && a.make_pcrelate) { std::fputs(kPcrelateNeedsResident, stderr); return 1; }
    if (streamed && !a.assoc_pheno.empty()) { std::fputs(kAssocNeedsResident, stderr); return 1; }
    if (streamed && !a.qtl_pheno.empty()) { std::fputs(kQtlNeedsResident, stderr); return 1; }
    if (streamed && !a.within.empty() && a.strat_asked()) { std::fputs(kStratNeedsResident, stderr); return 1; }
    if (streamed && a.sample_qc_asked()) { std::fputs(kSampleQcNeedsResident, stderr); return 1; }
    if (streamed && a.homozyg) { std::fputs(kHomozygNeedsResident, stderr); return 1; }
    if (streamed && !a.ld_score.empty()) { std::fputs(kLdScoreNeedsResident, stderr); return 1; }
    if (streamed && a.admixture) { std::fputs(kAdmixNeedsResident, stderr); return 1; }
    const gpca::SnpStats st = eng.snp_stats(gpca::QcConfig{a.min_call_rate, a.min_maf, a.max_hwe_p});
    std::vector<uint8_t> qc_pass;                                                                                       // empty: no sample filter
    if (a.sample_qc_asked() && !sample_ids.empty() && std::count(st.keep.begin(), st.keep.end(), (uint8_t)1) > 0) {
        std::vector<std::string> fids = fs.family_ids;
        if (use_kept) { fids.clear(); for (int64_t c : kept.cols) fids.push_back(fs.family_ids[(size_t)c]); }
        const int rc = run_sample_qc(eng, a, fids, sample_ids, st, qc_pass);
        if (rc != 0) return rc;
    }
    if (a.homozyg && !sample_ids.empty() && std::count(st.keep.begin(), st.keep.end(), (uint8_t)1) > 0) {
        std::vector<std::string> fids = fs.family_ids;
        if (use_kept) { fids.clear(); for (int64_t c : kept.cols) fids.push_back(fs.family_ids[(size_t)c]); }
        const int rc = run_homozyg(eng, a, fs, fids, sample_ids, st);
        if (rc != 0) return rc;
    }
    const auto blocks = gpca_host::parse_ld_block_file(a.ld_block_file);
    std::vector<uint8_t> keep;
    auto by_tag = gpca_host::map_snps_to_ld_blocks(blocks, fs.chromosomes, fs.positions, st.keep, keep);
    int64_t n_qc = 0, n_in = 0;
    for (uint8_t k : st.keep) n_qc += k;
    for (uint8_t k : keep) n_in += k;
    char buf[256];
    std::snprintf(buf, sizeof buf, "%lld / %zu SNPs passed QC; %lld fall in %zu LD blocks", (long long)n_qc, st.keep.size(), (long long)n_in, by_tag.size());
    logmsg(buf);
    if (sample_ids.empty() || n_in == 0) { logmsg("No samples or SNPs available for EigenSNP PCA after preparation."); return 0; }   // main.rs:349-352
    eng.set_standardization(st.mu, st.sigma, keep);
    if (a.have_indep) {
        // the threshold bits of the windowed r^2 in row bands, the pruning rule, P.prune.in / .out; the in-set narrows the keep mask
        // (mu, sigma unchanged) and the block lists (cli.py:_indep_pairwise)
        std::vector<int64_t> rows, pos;
        std::vector<std::string> chrom, ids;
        for (size_t i = 0; i < keep.size(); ++i)
            if (keep[i]) { rows.push_back((int64_t)i); chrom.push_back(fs.chromosomes[i]); pos.push_back(fs.positions[i]); ids.push_back(fs.variant_ids[i]); }
        std::vector<int64_t> win_end;
        try { win_end = gpca_host::ld_windows(chrom, pos, a.indep_window); }
        catch (const std::runtime_error& e) {
            std::fprintf(stderr, "error: --gpca-indep-pairwise: %s (variant indices count the SNPs kept by QC and the LD blocks)\n", e.what());
            return 1;
        }
        const std::vector<uint32_t> counts = eng.snp_qc_counts();
        std::vector<double> maf(rows.size());
        for (size_t t = 0; t < rows.size(); ++t) {
            const uint32_t* c = counts.data() + 4 * (size_t)rows[t];
            maf[t] = gpca_host::maf_from_counts(c[0], c[2], c[3]);
        }
        std::vector<uint8_t> in_ld(rows.size(), 1);
        for (int64_t r0 = 0; r0 < (int64_t)rows.size();) {
            int64_t r1 = 0, wm = 1;
            gpca_host::ld_next_band(win_end, r0, (int64_t)1 << 26, r1, wm);
            const std::vector<int64_t> we(win_end.begin() + r0, win_end.begin() + r1);
            std::vector<uint64_t> above;
            try { eng.ld_window(r0, r1, we, (int32_t)wm, a.indep_r2, nullptr, nullptr, &above); }
            catch (const gpca::Error& e) {
                if (e.status() != GPCA_ERR_STATE) throw;
                std::fprintf(stderr, "error: --gpca-indep-pairwise needs the genotype matrix resident on the device: with the matrix walked out "
                                     "of core a window crosses the panels, and the halo of rows that needs is not implemented\n");
                return 1;
            }
            gpca_host::ld_prune_band(win_end, r0, r1, above, (wm + 63) / 64, maf, in_ld);
            r0 = r1;
        }
        gpca_host::ensure_parent(a.output_prefix);
        gpca_host::write_prune_ids(a.output_prefix, ids, in_ld);
        int64_t n_ld = 0;
        for (uint8_t v : in_ld) n_ld += v;
        std::snprintf(buf, sizeof buf, "LD pruning (window %s, r^2 > %g): %lld SNPs kept, %lld removed", a.indep_window.c_str(), a.indep_r2, (long long)n_ld,
                      (long long)((int64_t)rows.size() - n_ld));
        logmsg(buf);
        std::fill(keep.begin(), keep.end(), (uint8_t)0);
        for (size_t t = 0; t < rows.size(); ++t) if (in_ld[t]) keep[(size_t)rows[t]] = 1;
        eng.set_standardization(st.mu, st.sigma, keep);
        for (auto& tr : by_tag) {
            auto& rs = tr.second;
            rs.erase(std::remove_if(rs.begin(), rs.end(), [&](int64_t r) { return !keep[(size_t)r]; }), rs.end());
        }
        by_tag.erase(std::remove_if(by_tag.begin(), by_tag.end(), [](const auto& tr) { return tr.second.empty(); }), by_tag.end());
        n_in = n_ld;
    }
    if (a.make_grm) {
        gpca_host::ensure_parent(a.output_prefix);
        std::vector<std::string> fids = fs.family_ids;
        if (use_kept) { fids.clear(); for (int64_t c : kept.cols) fids.push_back(fs.family_ids[(size_t)c]); }
        gpca_host::GrmWriter w(a.output_prefix, fids, sample_ids);
        const int scaling = a.grm_scaling == "centred" ? GPCA_GRM_CENTRED : GPCA_GRM_STANDARDIZED;
        const int64_t n = (int64_t)sample_ids.size();
        for (int64_t r0 = 0; r0 < n;) {      // row bands of at most 2^26 entries (at least one row), as the Python command line cuts them
            int64_t r1 = r0 + 1;
            while (r1 < n && (r1 + 1) * (r1 + 2) / 2 - r0 * (r0 + 1) / 2 <= ((int64_t)1 << 26)) ++r1;
            std::vector<float> np;
            const std::vector<double> g = eng.grm(scaling, r0, r1, &np);
            w.add_band(g.data(), np.data(), g.size());
            r0 = r1;
        }
        w.close();
        std::snprintf(buf, sizeof buf, "GRM of %lld samples over %lld SNPs written to %s.grm.bin", (long long)n, (long long)n_in, a.output_prefix.c_str());
        logmsg(buf);
    }
    std::vector<uint8_t> inset;
    if (a.make_king || a.have_king_cutoff) {
        // one pass over the bands of the kinship triangle: P.kin0 and / or the pairs above the cutoff (cli.py:_king)
        gpca_host::ensure_parent(a.output_prefix);
        std::vector<std::string> fids = fs.family_ids;
        if (use_kept) { fids.clear(); for (int64_t c : kept.cols) fids.push_back(fs.family_ids[(size_t)c]); }
        const int64_t n = (int64_t)sample_ids.size();
        std::unique_ptr<gpca_host::Kin0Writer> w;
        if (a.make_king) w.reset(new gpca_host::Kin0Writer(a.output_prefix, fids, sample_ids, a.have_king_filter, a.king_filter));
        std::vector<std::pair<int64_t, int64_t>> related;
        for (int64_t r0 = 0; r0 < n;) {      // row bands of at most 2^26 pairs (at least one row), as io.king_bands cuts them
            int64_t r1 = r0 + 1;
            while (r1 < n && (r1 + 1) * r1 / 2 - r0 * (r0 - 1) / 2 <= ((int64_t)1 << 26)) ++r1;
            std::vector<int32_t> cnt;
            const std::vector<double> kin = eng.king(r0, r1, &cnt);
            if (w) w->add_band(r0, r1, kin.data(), cnt.data());
            if (a.have_king_cutoff) {
                size_t i = 0;
                for (int64_t j = r0; j < r1; ++j)
                    for (int64_t k = 0; k < j; ++k, ++i)
                        if (kin[i] > a.king_cutoff) related.emplace_back(k, j);
            }
            r0 = r1;
        }
        if (w) {
            w->close(); w.reset();
            std::snprintf(buf, sizeof buf, "KING-robust kinship of %lld samples over %lld SNPs written to %s.kin0", (long long)n, (long long)n_in, a.output_prefix.c_str());
            logmsg(buf);
        }
        if (a.have_king_cutoff) {
            // a pair that touches a sample the sample QC failed is dropped before the greedy rule: a failed sample evicts no relative
            if (!qc_pass.empty())
                related.erase(std::remove_if(related.begin(), related.end(),
                                             [&](const std::pair<int64_t, int64_t>& p) { return !qc_pass[(size_t)p.first] || !qc_pass[(size_t)p.second]; }),
                              related.end());
            inset = gpca_host::king_unrelated(n, related);
            gpca_host::write_king_cutoff_ids(a.output_prefix, fids, sample_ids, inset);
            int64_t n_fit = 0;
            for (uint8_t v : inset) n_fit += v;
            std::snprintf(buf, sizeof buf, "KING cutoff %g: %zu related pairs, %lld of %lld samples left out of the fit", a.king_cutoff, related.size(),
                          (long long)(n - n_fit), (long long)n);
            logmsg(buf);
            if (n_fit < 2) { std::fprintf(stderr, "error: --gpca-king-cutoff leaves fewer than 2 samples to fit the PCA on\n"); return 1; }
        }
    }
    int64_t n_fit = (int64_t)sample_ids.size();
    if (!qc_pass.empty()) {                                                                                             // the in-set is KING's and the sample QC's
        if (inset.empty()) inset = qc_pass;
        else for (size_t i = 0; i < inset.size(); ++i) inset[i] = inset[i] && qc_pass[i];
    }
    if (!inset.empty()) { n_fit = 0; for (uint8_t v : inset) n_fit += v; }
    if (!qc_pass.empty() && n_fit < 2) { std::fprintf(stderr, "error: --gpca-mind / --gpca-het-sd leave fewer than 2 samples to fit the PCA on\n"); return 1; }
    gpca::MicroarrayGenotypeAccessor acc(eng);
    const std::vector<int64_t> rows = acc.original_indices_of_pca_snps();
    std::unordered_map<int64_t, int64_t> row_to_id;
    row_to_id.reserve(rows.size() * 2);
    for (size_t i = 0; i < rows.size(); ++i) row_to_id[rows[i]] = (int64_t)i;
    std::vector<gpca::LdBlockSpecification> specs;
    for (const auto& tr : by_tag) {
        gpca::LdBlockSpecification s; s.user_defined_block_tag = tr.first;
        for (int64_t r : tr.second) s.pca_snp_ids_in_block.push_back(row_to_id.at(r));
        specs.push_back(std::move(s));
    }
    gpca::EigenSNPCoreAlgorithmConfig cfg;
    const int64_t lim = std::min<int64_t>(n_fit, (int64_t)rows.size());
    const int64_t k = std::min<int64_t>(a.k_global, lim);
    cfg.target_num_global_pcs = (int)k;
    cfg.components_per_ld_block = (int)a.components_per_block;
    cfg.subset_factor_for_local_basis_learning = a.subset_factor;
    cfg.min_subset_size_for_local_basis_learning = a.min_subset; cfg.max_subset_size_for_local_basis_learning = a.max_subset;
    cfg.global_pca_sketch_oversampling = (int)std::max<int64_t>(0, std::min<int64_t>(a.global_oversampling, lim - k));
    cfg.global_pca_num_power_iterations = (int)a.global_power_iter;
    cfg.local_rsvd_sketch_oversampling = (int)a.local_oversampling; cfg.local_rsvd_num_power_iterations = (int)a.local_power_iter;
    cfg.random_seed = a.seed; cfg.snp_processing_strip_size = a.strip_size; cfg.refine_pass_count = (int)a.refine_passes;
    cfg.collect_diagnostics = a.collect_diagnostics;
    if (a.make_pcrelate && a.pcrelate_pcs > k) {
        std::fprintf(stderr, "error: --gpca-make-pcrelate %lld asks for more PCs than the %lld this run computes\n", (long long)a.pcrelate_pcs, (long long)k);
        return 1;
    }
    if (a.have_assoc_pcs && a.assoc_pcs > k) {
        std::fprintf(stderr, "error: --gpca-assoc-pcs %lld asks for more PCs than the %lld this run computes\n", (long long)a.assoc_pcs, (long long)k);
        return 1;
    }
    if (a.have_qtl_pcs && a.qtl_pcs > k) {
        std::fprintf(stderr, "error: --gpca-qtl-pcs %lld asks for more PCs than the %lld this run computes\n", (long long)a.qtl_pcs, (long long)k);
        return 1;
    }
    if (!inset.empty() && n_fit < (int64_t)inset.size()) eng.set_sample_mask(&inset);      // the fit sees the in-set only
    // with the cutoff every sample is projected onto the in-set's PCs (the relatives included), inside compute_pca while the fit is valid
    const gpca::EigenSNPCoreOutput out = gpca::EigenSNPCoreAlgorithm(cfg).compute_pca(acc, specs, a.local_stage, !inset.empty());
    const std::vector<double>& projected = out.projected_sample_scores;
    // the column count comes from the result: the local stage may leave fewer than k components (min(k, condensed features))
    const int kc = (int)out.num_principal_components_computed;
    gpca_host::ensure_parent(a.output_prefix);
    if (inset.empty())
        gpca_host::write_principal_components(a.output_prefix, "eigensnp.pca.tsv", sample_ids, out.final_sample_principal_component_scores.data(),
                                              out.num_qc_samples_used, kc);
    else
        gpca_host::write_principal_components(a.output_prefix, "eigensnp.pca.tsv", sample_ids, projected.data(), (int64_t)sample_ids.size(), kc);
    gpca_host::write_eigenvalues(a.output_prefix, out.final_principal_component_eigenvalues);
    std::vector<std::string> vids, chroms; std::vector<int64_t> pos;
    vids.reserve(rows.size()); chroms.reserve(rows.size()); pos.reserve(rows.size());
    for (int64_t r : rows) { vids.push_back(fs.variant_ids[(size_t)r]); chroms.push_back(fs.chromosomes[(size_t)r]); pos.push_back(fs.positions[(size_t)r]); }
    gpca_host::write_loadings(a.output_prefix, vids, chroms, pos, out.final_snp_principal_component_loadings.data(), (int64_t)rows.size(), kc);
    if (a.save_model) {
        gpca_host::ProjectionModel m;
        m.variant_ids = vids; m.chromosomes = chroms; m.positions = pos; m.k = kc; m.n_samples = n_fit;
        for (int64_t r : rows) {
            m.allele1.push_back(fs.allele1[(size_t)r]); m.allele2.push_back(fs.allele2[(size_t)r]);
            m.mean.push_back(st.mu[(size_t)r]); m.sd.push_back(st.sigma[(size_t)r]);
        }
        m.loadings.assign(out.final_snp_principal_component_loadings.begin(), out.final_snp_principal_component_loadings.begin() + rows.size() * (size_t)kc);
        m.eigenvalues = out.final_principal_component_eigenvalues;
        gpca_host::write_model(a.output_prefix, m);
    }
    if (a.admixture) {                                                                     // while the handle carries the PCA's keep mask
        std::vector<std::string> fids = fs.family_ids;
        if (use_kept) { fids.clear(); for (int64_t c : kept.cols) fids.push_back(fs.family_ids[(size_t)c]); }
        const int rc = run_admix(eng, a, fids, sample_ids, vids, inset);
        if (rc) return rc;
    }
    if (a.make_pcrelate) {
        // the bands of the PC-Relate triangle into P.pcrelate.kin / P.pcrelate.inbreed: V = the first P columns of the scores written above,
        // the regression fitted on the KING in-set when there is one, else on everyone (cli.py:_pcrelate)
        std::vector<std::string> fids = fs.family_ids;
        if (use_kept) { fids.clear(); for (int64_t c : kept.cols) fids.push_back(fs.family_ids[(size_t)c]); }
        const int64_t n = (int64_t)sample_ids.size();
        const int32_t P = (int32_t)a.pcrelate_pcs;
        std::vector<double> V((size_t)n * (size_t)P + 1);
        for (int64_t s = 0; s < n; ++s)
            for (int32_t c = 0; c < P; ++c)
                V[(size_t)s * P + c] = inset.empty() ? (double)out.final_sample_principal_component_scores[(size_t)s * kc + c] : projected[(size_t)s * kc + c];
        gpca_host::PcrelateWriter w(a.output_prefix, fids, sample_ids, a.have_pcrelate_filter, a.pcrelate_filter);
        try {
            for (int64_t r0 = 0; r0 < n;) {      // row bands of at most 2^26 entries (at least one row), as io.pcrelate_bands cuts them
                int64_t r1 = r0 + 1;
                while (r1 < n && (r1 + 1) * (r1 + 2) / 2 - r0 * (r0 + 1) / 2 <= ((int64_t)1 << 26)) ++r1;
                std::vector<int32_t> cnt;
                const std::vector<double> kin = eng.pcrelate(V, P, inset.empty() ? nullptr : &inset, a.pcrelate_tau, r0, r1, &cnt);
                w.add_band(r0, r1, kin.data(), cnt.data());
                r0 = r1;
            }
        } catch (const gpca::Error& e) {
            if (e.status() != GPCA_ERR_STATE) throw;
            std::fputs(kPcrelateNeedsResident, stderr);
            return 1;
        }
        w.close();
        std::snprintf(buf, sizeof buf, "PC-Relate kinship of %lld samples over %zu SNPs, adjusted for %d PCs, written to %s.pcrelate.kin", (long long)n,
                      rows.size(), (int)P, a.output_prefix.c_str());
        logmsg(buf);
    }
    if (!a.within.empty() && a.strat_asked()) {
        std::vector<std::string> fids = fs.family_ids;
        if (use_kept) { fids.clear(); for (int64_t c : kept.cols) fids.push_back(fs.family_ids[(size_t)c]); }
        const int rc = run_strat(eng, a, fs, fids, sample_ids, st);
        if (rc) return rc;
    }
    std::vector<double> l2;
    if (!a.ld_score.empty()) {
        const int rc = run_ld_score(eng, a, fs, st, l2);
        if (rc) return rc;
    }
    if (!a.assoc_pheno.empty()) {
        std::vector<std::string> fids = fs.family_ids;
        if (use_kept) { fids.clear(); for (int64_t c : kept.cols) fids.push_back(fs.family_ids[(size_t)c]); }
        std::vector<double> scores = projected;
        if (inset.empty()) scores.assign(out.final_sample_principal_component_scores.begin(), out.final_sample_principal_component_scores.end());
        const int rc = run_assoc(eng, a, fs, fids, sample_ids, scores, kc, inset, st, l2);
        if (rc) return rc;
    }
    if (!a.qtl_pheno.empty()) {
        std::vector<std::string> fids = fs.family_ids;
        if (use_kept) { fids.clear(); for (int64_t c : kept.cols) fids.push_back(fs.family_ids[(size_t)c]); }
        std::vector<double> scores = projected;
        if (inset.empty()) scores.assign(out.final_sample_principal_component_scores.begin(), out.final_sample_principal_component_scores.end());
        const int rc = run_qtl(eng, a, fs, fids, sample_ids, scores, kc, inset, st);
        if (rc) return rc;
    }
    std::snprintf(buf, sizeof buf, "EigenSNP workflow done in %.2fs", seconds_since(t0));
    logmsg(buf);
    return 0;
}

// ------------------------------------------------------------------------------------------------ projection onto a fitted model
// --gpca-project-model MODEL --bed-file TARGET --out Q: the target's samples on the model's PCs (gpca_project; cli.py:run_project_workflow)
int run_project_workflow(Args a) {
    auto refuse = [](const char* m) { std::fprintf(stderr, "error: %s\n", m); return 2; };
    if (a.bed_file.empty()) return refuse("--bed-file is required with --gpca-project-model");
    if (a.eigensnp || !a.vcf_dir.empty()) return refuse("--gpca-project-model takes a --bed-file target, not --eigensnp or --vcf-dir");
    if (a.precision != "i8") return refuse("--gpca-project-model needs --gpca-precision i8");
    const auto t0 = std::chrono::steady_clock::now();
    const gpca_host::ProjectionModel model = gpca_host::read_model(a.project_model);
    gpca_host::PlinkFileset fs;
    gpca_host::read_plink(a.bed_file, fs);
    const gpca_host::Alignment al = gpca_host::align_model(model, fs.variant_ids, fs.allele1, fs.allele2);
    char buf[512];
    std::snprintf(buf, sizeof buf, "model of %zu SNPs, k = %d: %lld matched (%lld with swapped alleles), %lld allele mismatches dropped, %lld absent from the target",
                  model.variant_ids.size(), model.k, (long long)al.matched, (long long)al.flipped, (long long)al.allele_mismatch, (long long)al.absent);
    logmsg(buf);
    if (al.matched == 0) {
        std::fprintf(stderr, "error: no SNP of %s matches a variant of %s (by ID and alleles)\n", a.project_model.c_str(), a.bed_file.c_str());
        return 1;
    }
    const int store = engine_storage(a, fs.n_samples);
    gpca::Engine eng(a.device, engine_precision(a), store);
    load_bed(eng, a, fs, nullptr);
    std::vector<int32_t> used;
    const std::vector<double> scores = eng.project(al.mean.data(), al.sd.data(), al.loadings.data(), model.k, &used);
    gpca_host::ensure_parent(a.output_prefix);
    gpca_host::write_projected(a.output_prefix, fs.sample_ids, scores.data(), model.k, used);
    std::snprintf(buf, sizeof buf, "projection of %lld samples done in %.2fs", (long long)fs.n_samples, seconds_since(t0));
    logmsg(buf);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    Args a = parse(argc, argv);
    try {
        if (a.have_indep) {
            if (!a.eigensnp) { std::fprintf(stderr, "error: --gpca-indep-pairwise needs the --eigensnp workflow\n"); return 2; }
            try { gpca_host::parse_ld_window(a.indep_window); }
            catch (const std::runtime_error& e) { std::fprintf(stderr, "error: --gpca-indep-pairwise: %s\n", e.what()); return 2; }
            char* end = nullptr;
            a.indep_r2 = a.indep_r2_text.empty() ? std::nan("") : std::strtod(a.indep_r2_text.c_str(), &end);
            if ((end && *end) || !(a.indep_r2 > 0.0 && a.indep_r2 < 1.0)) { std::fprintf(stderr, "error: --gpca-indep-pairwise R2 must lie in (0, 1)\n"); return 2; }
        }
        if (a.make_grm && !a.eigensnp) { std::fprintf(stderr, "error: --gpca-make-grm needs the --eigensnp workflow\n"); return 2; }
        if ((a.make_king || a.have_king_cutoff) && !a.eigensnp) { std::fprintf(stderr, "error: --gpca-make-king and --gpca-king-cutoff need the --eigensnp workflow\n"); return 2; }
        if (a.have_king_filter && !a.make_king) { std::fprintf(stderr, "error: --gpca-king-table-filter needs --gpca-make-king\n"); return 2; }
        if (a.have_king_cutoff && !(a.king_cutoff > 0.0 && a.king_cutoff < 0.5)) { std::fprintf(stderr, "error: --gpca-king-cutoff must lie in (0, 0.5)\n"); return 2; }
        if (a.have_king_cutoff && a.local_stage) {
            std::fprintf(stderr, "error: --gpca-king-cutoff cannot be combined with --gpca-eigensnp-local-stage (that stage owns the sample mask)\n");
            return 2;
        }
        if (!a.make_pcrelate && (a.have_pcrelate_tau || a.have_pcrelate_filter)) {
            std::fprintf(stderr, "error: --gpca-pcrelate-maf-bound and --gpca-pcrelate-table-filter need --gpca-make-pcrelate\n");
            return 2;
        }
        if (a.make_pcrelate) {
            if (!a.eigensnp) { std::fprintf(stderr, "error: --gpca-make-pcrelate needs the --eigensnp workflow\n"); return 2; }
            if (!(a.pcrelate_pcs >= 0 && a.pcrelate_pcs <= std::min<int64_t>(a.k_global, 32))) {
                std::fprintf(stderr, "error: --gpca-make-pcrelate P must lie in [0, min(--eigensnp-k-global, 32)]\n");
                return 2;
            }
            if (!(a.pcrelate_tau >= 0.0 && a.pcrelate_tau < 0.5)) { std::fprintf(stderr, "error: --gpca-pcrelate-maf-bound must lie in [0, 0.5)\n"); return 2; }
            if (a.local_stage) {
                std::fprintf(stderr, "error: --gpca-make-pcrelate cannot be combined with --gpca-eigensnp-local-stage (that stage defines no all-sample scores)\n");
                return 2;
            }
            if (a.stream == "on") { std::fputs(kPcrelateNeedsResident, stderr); return 2; }
        }
        if (a.assoc_pheno.empty() && (a.have_assoc_pcs || !a.assoc_covar.empty() || a.have_assoc_vif)) {
            std::fprintf(stderr, "error: --gpca-assoc-pcs, --gpca-assoc-covar and --gpca-assoc-vif need --gpca-assoc-pheno\n");
            return 2;
        }
        if (a.assoc_logistic && a.assoc_pheno.empty()) { std::fprintf(stderr, "error: --gpca-assoc-logistic needs --gpca-assoc-pheno\n"); return 2; }
        if (a.assoc_spa && !a.assoc_logistic) { std::fprintf(stderr, "error: --gpca-assoc-spa needs --gpca-assoc-logistic\n"); return 2; }
        if (a.have_assoc_spa_z && !a.assoc_spa) { std::fprintf(stderr, "error: --gpca-assoc-spa-z needs --gpca-assoc-spa\n"); return 2; }
        if (a.have_assoc_spa_z && !gpca_host::spa_z_ok(a.assoc_spa_z)) {
            std::fprintf(stderr, "error: --gpca-assoc-spa-z must be at least 0.5, or inf for no correction\n");
            return 2;
        }
        if (a.assoc_firth && !a.assoc_logistic) { std::fprintf(stderr, "error: --gpca-assoc-firth needs --gpca-assoc-logistic\n"); return 2; }
        if (a.assoc_firth && a.assoc_spa) { std::fprintf(stderr, "error: --gpca-assoc-firth and --gpca-assoc-spa exclude each other\n"); return 2; }
        if (a.have_assoc_firth_z && !a.assoc_firth) { std::fprintf(stderr, "error: --gpca-assoc-firth-z needs --gpca-assoc-firth\n"); return 2; }
        if (a.have_assoc_firth_z && !gpca_host::firth_z_ok(a.assoc_firth_z)) {
            std::fprintf(stderr, "error: --gpca-assoc-firth-z must be at least 0, or inf for no correction\n");
            return 2;
        }
        if (!a.assoc_set_list.empty() && !a.assoc_logistic) { std::fprintf(stderr, "error: --gpca-assoc-set-list needs --gpca-assoc-logistic\n"); return 2; }
        if (a.assoc_set_list.empty() && (a.have_assoc_set_max_maf || a.have_assoc_set_weights)) {
            std::fprintf(stderr, "error: --gpca-assoc-set-max-maf and --gpca-assoc-set-weights need --gpca-assoc-set-list\n");
            return 2;
        }
        if (a.have_assoc_set_max_maf && !(a.assoc_set_max_maf > 0.0 && a.assoc_set_max_maf <= 0.5)) {
            std::fprintf(stderr, "error: --gpca-assoc-set-max-maf must lie in (0, 0.5]\n");
            return 2;
        }
        if (a.have_assoc_set_weights && a.assoc_set_weights != "beta" && a.assoc_set_weights != "flat") {
            std::fprintf(stderr, "error: --gpca-assoc-set-weights must be beta or flat\n");
            return 2;
        }
        if (a.assoc_cc_freq && !a.assoc_logistic) { std::fprintf(stderr, "error: --gpca-assoc-cc-freq needs --gpca-assoc-logistic\n"); return 2; }
        if (a.within.empty() && (a.freq_strat || a.have_fst)) { std::fprintf(stderr, "error: --gpca-freq-strat and --gpca-fst need --gpca-within\n"); return 2; }
        if (a.within.empty() && (a.fstat_asked() || a.have_fstat_block)) {
            std::fprintf(stderr, "error: --gpca-f2, --gpca-fstats and --gpca-fstat-block need --gpca-within\n");
            return 2;
        }
        if (a.have_fstat_block && !a.fstat_asked()) { std::fprintf(stderr, "error: --gpca-fstat-block needs --gpca-f2 or --gpca-fstats\n"); return 2; }
        if (a.fstat_asked()) {
            try { gpca_host::parse_ld_window(a.fstat_block); }
            catch (const std::runtime_error&) {
                std::fprintf(stderr, "error: --gpca-fstat-block: '%s' is neither a variant count such as 500 nor a span such as 5000kb\n", a.fstat_block.c_str());
                return 2;
            }
        }
        if (a.fst_variants && !a.have_fst) { std::fprintf(stderr, "error: --gpca-fst-variants needs --gpca-fst\n"); return 2; }
        if (a.have_fst && a.fst != "hudson" && a.fst != "wc") { std::fprintf(stderr, "error: --gpca-fst must be hudson or wc\n"); return 2; }
        if (!a.within.empty()) {
            if (!a.eigensnp) { std::fprintf(stderr, "error: --gpca-within needs the --eigensnp workflow\n"); return 2; }
            if (!a.strat_asked() && !a.admix_supervised) { std::fprintf(stderr, "error: --gpca-within needs --gpca-freq-strat or --gpca-fst\n"); return 2; }
            if (a.stream == "on" && a.strat_asked()) { std::fputs(kStratNeedsResident, stderr); return 2; }
            try { a.within_table = gpca_host::read_within(a.within); }
            catch (const std::runtime_error& e) { std::fprintf(stderr, "error: --gpca-within: %s\n", e.what()); return 2; }
            const size_t ng = a.within_table.names.size();
            if ((int64_t)ng > gpca_host::kGroupsMax) {
                std::fprintf(stderr, "error: --gpca-within: %zu groups are more than %lld\n", ng, (long long)gpca_host::kGroupsMax);
                return 2;
            }
            if (a.have_fst && ng < 2) { std::fprintf(stderr, "error: --gpca-fst needs at least two groups, --gpca-within names %zu\n", ng); return 2; }
            if (a.fstat_asked() && ng < 2) {
                std::fprintf(stderr, "error: --gpca-f2 and --gpca-fstats need at least two groups, --gpca-within names %zu\n", ng);
                return 2;
            }
            if (ng < 1) { std::fprintf(stderr, "error: --gpca-within names no group\n"); return 2; }
            if (!a.fstats.empty()) {
                try { a.fstats_list = gpca_host::read_fstats_list(a.fstats, a.within_table.names); }
                catch (const std::runtime_error& e) { std::fprintf(stderr, "error: --gpca-fstats: %s\n", e.what()); return 2; }
            }
        }
        if (a.sample_qc_asked()) {
            if (!a.eigensnp) { std::fprintf(stderr, "error: --gpca-sample-missing, --gpca-het, --gpca-mind and --gpca-het-sd need the --eigensnp workflow\n"); return 2; }
            if (a.have_mind && !(a.mind >= 0.0 && a.mind < 1.0)) { std::fprintf(stderr, "error: --gpca-mind must lie in [0, 1)\n"); return 2; }
            if (a.have_het_sd && !(a.het_sd > 0.0 && std::isfinite(a.het_sd))) { std::fprintf(stderr, "error: --gpca-het-sd must be finite and above 0\n"); return 2; }
            if ((a.have_mind || a.have_het_sd) && a.local_stage) {
                std::fprintf(stderr, "error: --gpca-mind and --gpca-het-sd cannot be combined with --gpca-eigensnp-local-stage (that stage owns the sample mask)\n");
                return 2;
            }
            if (a.stream == "on") { std::fputs(kSampleQcNeedsResident, stderr); return 2; }
        }
        if (!a.admixture && a.admix_value_flag) {
            std::fprintf(stderr, "error: --gpca-admixture-seed, -max-iter, -tol, -no-accel and --gpca-admixture-supervised need --gpca-admixture\n");
            return 2;
        }
        if (a.admixture) {
            if (!a.eigensnp) { std::fprintf(stderr, "error: --gpca-admixture needs the --eigensnp workflow\n"); return 2; }
            if (!(a.admix_k >= 1 && a.admix_k <= GPCA_ADMIX_MAX_K)) { std::fprintf(stderr, "error: --gpca-admixture K must lie in [1, 16]\n"); return 2; }
            if (a.admix_seed < 0) { std::fprintf(stderr, "error: --gpca-admixture-seed must lie in [0, 2^63)\n"); return 2; }
            if (!(a.admix_max_iter >= 0 && a.admix_max_iter <= 2147483647LL)) { std::fprintf(stderr, "error: --gpca-admixture-max-iter must lie in [0, 2^31)\n"); return 2; }
            if (!(a.admix_tol >= 0.0 && a.admix_tol < HUGE_VAL)) { std::fprintf(stderr, "error: --gpca-admixture-tol must be finite and at least 0\n"); return 2; }
            if (a.admix_supervised) {
                if (a.within.empty()) { std::fprintf(stderr, "error: --gpca-admixture-supervised needs --gpca-within\n"); return 2; }
                if ((int64_t)a.within_table.names.size() != a.admix_k) {
                    std::fprintf(stderr, "error: --gpca-admixture-supervised: K = %lld but --gpca-within names %zu groups\n", (long long)a.admix_k, a.within_table.names.size());
                    return 2;
                }
            }
            if (a.local_stage) {
                std::fprintf(stderr, "error: --gpca-admixture cannot be combined with --gpca-eigensnp-local-stage (that stage owns the sample mask and the keep mask)\n");
                return 2;
            }
            if (a.stream == "on") { std::fputs(kAdmixNeedsResident, stderr); return 2; }
        }
        if (a.admix_cv || a.admix_cv_flag) {
            if (!a.admixture) { std::fprintf(stderr, "error: --gpca-admixture-cv, --gpca-admixture-cv-seed and --gpca-admixture-cv-k need --gpca-admixture\n"); return 2; }
            if (!a.admix_cv) { std::fprintf(stderr, "error: --gpca-admixture-cv-seed and --gpca-admixture-cv-k need --gpca-admixture-cv\n"); return 2; }
            if (!(a.admix_cv_folds >= 2 && a.admix_cv_folds <= GPCA_ADMIX_CV_MAX_FOLDS)) { std::fprintf(stderr, "error: --gpca-admixture-cv V must lie in [2, 64]\n"); return 2; }
            if (a.admix_cv_seed < 0) { std::fprintf(stderr, "error: --gpca-admixture-cv-seed must lie in [0, 2^63)\n"); return 2; }
            int lo = (int)a.admix_k, hi = (int)a.admix_k;
            if (!a.admix_cv_k.empty()) {
                if (a.admix_supervised) {
                    std::fprintf(stderr, "error: --gpca-admixture-cv-k cannot be combined with --gpca-admixture-supervised (the groups fix K)\n");
                    return 2;
                }
                const size_t dash = a.admix_cv_k.find('-');
                const std::string A = a.admix_cv_k.substr(0, dash), B = dash == std::string::npos ? "" : a.admix_cv_k.substr(dash + 1);
                auto digits = [](const std::string& t) { return !t.empty() && t.size() <= 2 && t.find_first_not_of("0123456789") == std::string::npos; };
                if (!digits(A) || !digits(B) || !(1 <= std::stoi(A) && std::stoi(A) <= std::stoi(B) && std::stoi(B) <= GPCA_ADMIX_MAX_K)) {
                    std::fprintf(stderr, "error: --gpca-admixture-cv-k must be A-B with 1 <= A <= B <= 16\n");
                    return 2;
                }
                lo = std::stoi(A); hi = std::stoi(B);
            }
            for (int k = std::min(lo, (int)a.admix_k); k <= std::max(hi, (int)a.admix_k); ++k)
                if ((k >= lo && k <= hi) || k == (int)a.admix_k) a.admix_cv_ks.push_back(k);
        }
        if (a.homozyg) {
            if (!a.eigensnp) { std::fprintf(stderr, "error: --gpca-homozyg needs the --eigensnp workflow\n"); return 2; }
            if (!(a.hom_window_snp >= 1 && a.hom_window_snp <= GPCA_ROH_WINDOW_MAX)) { std::fprintf(stderr, "error: --gpca-homozyg-window-snp must lie in [1, 64]\n"); return 2; }
            if (!(a.hom_window_het >= 0 && a.hom_window_het <= a.hom_window_snp && a.hom_window_missing >= 0 && a.hom_window_missing <= a.hom_window_snp)) {
                std::fprintf(stderr, "error: --gpca-homozyg-window-het and --gpca-homozyg-window-missing must lie in [0, --gpca-homozyg-window-snp]\n");
                return 2;
            }
            if (!gpca_host::roh_threshold(a.hom_threshold, a.hom_thr_num, a.hom_thr_den) || a.hom_thr_num > a.hom_thr_den) {
                std::fprintf(stderr, "error: --gpca-homozyg-window-threshold must be a decimal number in [0, 1] whose exact fraction has a denominator of at most 2^20\n");
                return 2;
            }
            if (!(a.hom_snp >= 1 && a.hom_snp <= 2147483647LL)) { std::fprintf(stderr, "error: --gpca-homozyg-snp must lie in [1, 2^31)\n"); return 2; }
            for (double v : {a.hom_kb, a.hom_density, a.hom_gap})
                if (!(v >= 0.0 && v <= 1e12)) {
                    std::fprintf(stderr, "error: --gpca-homozyg-kb, --gpca-homozyg-density and --gpca-homozyg-gap must lie in [0, 1e12]\n");
                    return 2;
                }
            if (a.have_hom_het && !(a.hom_het >= 0 && a.hom_het <= 2147483647LL)) { std::fprintf(stderr, "error: --gpca-homozyg-het must lie in [0, 2^31)\n"); return 2; }
            if (a.stream == "on") { std::fputs(kHomozygNeedsResident, stderr); return 2; }
        }
        if (!a.assoc_pheno.empty()) {
            if (!a.eigensnp) { std::fprintf(stderr, "error: --gpca-assoc-pheno needs the --eigensnp workflow\n"); return 2; }
            if (a.have_assoc_pcs && !(a.assoc_pcs >= 0 && a.assoc_pcs <= a.k_global)) {
                std::fprintf(stderr, "error: --gpca-assoc-pcs P must lie in [0, --eigensnp-k-global]\n");
                return 2;
            }
            if (!(a.assoc_vif >= 1.0) || !std::isfinite(a.assoc_vif)) { std::fprintf(stderr, "error: --gpca-assoc-vif must be finite and at least 1\n"); return 2; }
            if (a.local_stage) {
                std::fprintf(stderr, "error: --gpca-assoc-pheno cannot be combined with --gpca-eigensnp-local-stage (that stage defines no all-sample scores)\n");
                return 2;
            }
            if (a.stream == "on") { std::fputs(kAssocNeedsResident, stderr); return 2; }
            try { a.assoc_pheno_table = gpca_host::read_pheno(a.assoc_pheno); }
            catch (const std::runtime_error& e) { std::fprintf(stderr, "error: --gpca-assoc-pheno: %s\n", e.what()); return 2; }
            if (!a.assoc_covar.empty()) {
                try { a.assoc_covar_table = gpca_host::read_pheno(a.assoc_covar); }
                catch (const std::runtime_error& e) { std::fprintf(stderr, "error: --gpca-assoc-covar: %s\n", e.what()); return 2; }
            }
            int64_t t = (int64_t)a.assoc_pheno_table.names.size();
            const int64_t c = (int64_t)a.assoc_covar_table.names.size(), p = a.have_assoc_pcs ? a.assoc_pcs : a.k_global;
            if (a.assoc_logistic) {
                int64_t nb = 0;
                for (size_t j = 0; j < a.assoc_pheno_table.names.size(); ++j) nb += gpca_host::binary_trait(a.assoc_pheno_table, j, nullptr);
                if (nb && p + c + 3 > kAssocMaxColumns) {
                    std::fprintf(stderr, "error: --gpca-assoc-logistic: %lld PCs + %lld covariates + 3 are more than %lld columns\n", (long long)p, (long long)c,
                                 (long long)kAssocMaxColumns);
                    return 2;
                }
                t -= nb;                                                              // the linear scan takes the quantitative traits
            }
            if (t + p + c > kAssocMaxColumns) {
                std::fprintf(stderr, "error: --gpca-assoc-pheno: %lld traits + %lld PCs + %lld covariates are more than %lld columns\n", (long long)t, (long long)p,
                             (long long)c, (long long)kAssocMaxColumns);
                return 2;
            }
            if (!a.assoc_set_list.empty()) {                                          // (its format, before any work on the device)
                try { gpca_host::read_set_list(a.assoc_set_list, {}); }
                catch (const std::runtime_error& e) { std::fprintf(stderr, "error: --gpca-assoc-set-list: %s\n", e.what()); return 2; }
            }
        }
        if (a.qtl_pheno.empty() && (a.have_qtl_pcs || !a.qtl_covar.empty() || a.have_qtl_log10p || a.have_qtl_t || a.have_qtl_vif)) {
            std::fprintf(stderr, "error: --gpca-qtl-pcs, --gpca-qtl-covar, --gpca-qtl-log10p, --gpca-qtl-t and --gpca-qtl-vif need --gpca-qtl-pheno\n");
            return 2;
        }
        if (!a.qtl_pheno.empty()) {
            if (!a.eigensnp) { std::fprintf(stderr, "error: --gpca-qtl-pheno needs the --eigensnp workflow\n"); return 2; }
            if (a.have_qtl_pcs && !(a.qtl_pcs >= 0 && a.qtl_pcs <= a.k_global)) {
                std::fprintf(stderr, "error: --gpca-qtl-pcs P must lie in [0, --eigensnp-k-global]\n");
                return 2;
            }
            if (!(a.qtl_vif >= 1.0) || !std::isfinite(a.qtl_vif)) { std::fprintf(stderr, "error: --gpca-qtl-vif must be finite and at least 1\n"); return 2; }
            if (a.have_qtl_log10p && a.have_qtl_t) { std::fprintf(stderr, "error: --gpca-qtl-log10p and --gpca-qtl-t set the same threshold: give one\n"); return 2; }
            if (!(a.qtl_log10p >= 0.0) || !std::isfinite(a.qtl_log10p)) { std::fprintf(stderr, "error: --gpca-qtl-log10p must be finite and at least 0\n"); return 2; }
            if (!(a.qtl_t >= 0.0) || !std::isfinite(a.qtl_t)) { std::fprintf(stderr, "error: --gpca-qtl-t must be finite and at least 0\n"); return 2; }
            if (a.local_stage) {
                std::fprintf(stderr, "error: --gpca-qtl-pheno cannot be combined with --gpca-eigensnp-local-stage (that stage defines no all-sample scores)\n");
                return 2;
            }
            if (a.stream == "on") { std::fputs(kQtlNeedsResident, stderr); return 2; }
            try { a.qtl_pheno_table = gpca_host::read_pheno(a.qtl_pheno); }
            catch (const std::runtime_error& e) { std::fprintf(stderr, "error: --gpca-qtl-pheno: %s\n", e.what()); return 2; }
            if (!a.qtl_covar.empty()) {
                try { a.qtl_covar_table = gpca_host::read_pheno(a.qtl_covar); }
                catch (const std::runtime_error& e) { std::fprintf(stderr, "error: --gpca-qtl-covar: %s\n", e.what()); return 2; }
            }
            const int64_t t = (int64_t)a.qtl_pheno_table.names.size(), c = (int64_t)a.qtl_covar_table.names.size(), p = a.have_qtl_pcs ? a.qtl_pcs : a.k_global;
            if (t > kQtlMaxTraits) { std::fprintf(stderr, "error: --gpca-qtl-pheno: %lld traits are more than %lld\n", (long long)t, (long long)kQtlMaxTraits); return 2; }
            if (p + c > kQtlMaxCovariates) {
                std::fprintf(stderr, "error: --gpca-qtl-pheno: %lld PCs + %lld covariates are more than %lld covariates\n", (long long)p, (long long)c,
                             (long long)kQtlMaxCovariates);
                return 2;
            }
        }
        if (a.qtl_cis_pos.empty() && (a.qtl_cis_only || a.have_qtl_cis_window || a.have_qtl_cis_perm || a.have_qtl_cis_seed)) {
            std::fprintf(stderr, "error: --gpca-qtl-cis-window, --gpca-qtl-cis-perm, --gpca-qtl-cis-seed and --gpca-qtl-cis-only need --gpca-qtl-cis-pos\n");
            return 2;
        }
        if (!a.qtl_cis_pos.empty()) {
            if (a.qtl_pheno.empty()) { std::fprintf(stderr, "error: --gpca-qtl-cis-pos needs --gpca-qtl-pheno\n"); return 2; }
            if (a.qtl_cis_window < 0) { std::fprintf(stderr, "error: --gpca-qtl-cis-window must be at least 0\n"); return 2; }
            if (a.qtl_cis_perm < 0 || a.qtl_cis_perm > 65535) { std::fprintf(stderr, "error: --gpca-qtl-cis-perm must lie in [0, 65535]\n"); return 2; }
            if (a.qtl_cis_seed < 0) { std::fprintf(stderr, "error: --gpca-qtl-cis-seed must be at least 0\n"); return 2; }
            try { a.qtl_cis_table = gpca_host::read_trait_pos(a.qtl_cis_pos); }
            catch (const std::runtime_error& e) { std::fprintf(stderr, "error: --gpca-qtl-cis-pos: %s\n", e.what()); return 2; }
        }
        if (a.assoc_ldsc && (a.ld_score.empty() || a.assoc_pheno.empty())) {
            std::fprintf(stderr, "error: --gpca-assoc-ldsc needs --gpca-ld-score and --gpca-assoc-pheno\n");
            return 2;
        }
        if (!a.ld_score.empty()) {
            if (!a.eigensnp) { std::fprintf(stderr, "error: --gpca-ld-score needs the --eigensnp workflow\n"); return 2; }
            try { gpca_host::parse_ld_window(a.ld_score); }
            catch (const std::runtime_error& e) { std::fprintf(stderr, "error: --gpca-ld-score: %s\n", e.what()); return 2; }
            if (a.stream == "on") { std::fputs(kLdScoreNeedsResident, stderr); return 2; }
        }
        if (!a.project_model.empty()) return run_project_workflow(a);
        if (a.save_model && !a.eigensnp) { std::fprintf(stderr, "error: --gpca-save-model needs the --eigensnp workflow\n"); return 2; }
        return a.eigensnp ? run_eigensnp_workflow(a) : run_vcf_workflow(a);
    } catch (const gpca::Error& e) {
        std::fprintf(stderr, "Error: %s\n", e.what());
        return 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "Error: %s\n", e.what());
        return 1;
    }
}
