"""`python -m genomic_pca_amd` -- the reference's CLI surface (main.rs:501-593) over the MI355X engine.

Two workflows, dispatched on --eigensnp like main.rs:109-122:
  * VCF  (run_vcf_workflow, main.rs:133-247):  --vcf-dir D -k K [--maf f] [--rfit-seed s] --out P
        -> P.vcf.pca.tsv, P.eigenvalues.tsv (header only, as main.rs:676 leaves the vector empty;
           --write-eigenvalues is an extension that fills it)
  * BED  (run_eigensnp_rust_workflow, main.rs:250-442):  --eigensnp --bed-file B --ld-block-file L --out P [--eigensnp-*]
        -> P.eigensnp.pca.tsv, P.eigenvalues.tsv, P.eigensnp.loadings.tsv
EigenSNP's per-LD-block local stage is defined only in the un-vendored efficient_pca crate; this CLI runs the global
randomized PCA over all SNPs that pass QC and fall in an LD block (identical to the reference's own README usage of a
single genome-wide block) by default; --gpca-eigensnp-local-stage runs the multi-stage algorithm the local-stage / refine
flags parameterise, as published for that crate (parity unpinned).
"""
from __future__ import annotations

import argparse
import math
import os
import sys
import time

import numpy as np

from . import io as gio
from .engine import (EigenSNPCoreAlgorithm, EigenSNPCoreAlgorithmConfig, GpcaEngine, LdBlockSpecification,
                     MicroarrayGenotypeAccessor, PCA, QcConfig)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="genomic_pca", description="Genomic PCA Tool from VCF or BED/LD-block files.")
    p.add_argument("-o", "--out", dest="output_prefix", required=True, help="Output file prefix.")
    p.add_argument("-t", "--threads", type=int, default=None, help="accepted for compatibility (the GPU does the work)")
    p.add_argument("--log-level", default="Info")
    p.add_argument("-d", "--vcf-dir", default=None)
    p.add_argument("-k", "--components", type=int, default=None,
                   help="Number of principal components to compute (for VCF workflow); at most 118 here (the sketch holds components + 10 <= 128 "
                        "columns, gpca.h; the reference clamps only to min(samples, variants), main.rs:621-628)")
    p.add_argument("--maf", type=float, default=None)
    p.add_argument("--rfit-seed", type=int, default=None)
    p.add_argument("--eigensnp", action="store_true")
    p.add_argument("--bed-file", default=None)
    p.add_argument("--ld-block-file", default=None)
    p.add_argument("--eigensnp-sample-keep-file", default=None)
    # clap's effective defaults when --eigensnp is given (main.rs:545-588)
    p.add_argument("--eigensnp-min-call-rate", type=float, default=0.98)
    p.add_argument("--eigensnp-min-maf", type=float, default=0.01)
    p.add_argument("--eigensnp-max-hwe-p", type=float, default=1e-6)
    p.add_argument("--eigensnp-k-global", type=int, default=10)
    p.add_argument("--eigensnp-components-per-block", type=int, default=7)
    p.add_argument("--eigensnp-subset-factor", type=float, default=0.075)
    p.add_argument("--eigensnp-min-subset-size", type=int, default=10000)
    p.add_argument("--eigensnp-max-subset-size", type=int, default=40000)
    p.add_argument("--eigensnp-global-oversampling", type=int, default=10)
    p.add_argument("--eigensnp-global-power-iter", type=int, default=2)
    p.add_argument("--eigensnp-local-oversampling", type=int, default=10)
    p.add_argument("--eigensnp-local-power-iter", type=int, default=2)
    p.add_argument("--eigensnp-seed", type=int, default=2025)
    p.add_argument("--eigensnp-snp-strip-size", type=int, default=2000)
    p.add_argument("--eigensnp-refine-passes", type=int, default=1)
    p.add_argument("--eigensnp-collect-diagnostics", action="store_true")
    # extensions
    p.add_argument("--device", type=int, default=-1, help="HIP device ordinal")
    p.add_argument("--write-eigenvalues", action="store_true", help="VCF workflow: fill P.eigenvalues.tsv (the reference leaves it header-only)")
    # engine selection (extensions; the defaults are the path bench.py's headline times)
    p.add_argument("--gpca-precision", default="i8", choices=["i8", "f32"], help="i8 = exact-integer GEMMs (default); f32 = f32 matrix cores")
    p.add_argument("--gpca-storage", default="auto", choices=["auto", "int8", "2bit"],
                   help="HBM residency of the genotypes: int8 (1 B per genotype) or 2bit (PLINK-style codes, 0.25 B, faster from 1 024 "
                        "samples up); auto = 2bit for a .bed with at least 1 024 samples, int8 otherwise")
    p.add_argument("--gpca-stream", default="auto", choices=["auto", "on", "off"],
                   help="EigenSNP workflow: walk the .bed out of core through a ring of HBM panels instead of holding it resident "
                        "(auto = when the resident load runs out of device memory; needs --gpca-precision i8)")
    p.add_argument("--gpca-panel-rows", type=int, default=0, help="--gpca-stream: SNP rows per panel (0 = engine default)")
    p.add_argument("--gpca-rfit-power-iters", type=int, default=2,
                   help="VCF workflow: power iterations of the randomized PCA (PCA::rfit's own count is fixed inside the un-vendored "
                        "efficient_pca crate and unknown; 2 = the EigenSNP default, main.rs:318; 4 puts the PCs within 2e-6 of exact PCA)")
    p.add_argument("--gpca-eigensnp-local-stage", action="store_true",
                   help="EigenSNP workflow: run the multi-stage algorithm the --eigensnp-* local / refine flags parameterise (per-block "
                        "local bases on a sample subset, condensed features, global PCA, refinement) instead of one global randomized "
                        "PCA over all blocks (the default: fewer passes, more accurate); needs a resident matrix")
    # projection onto a fitted model (extensions)
    p.add_argument("--gpca-save-model", action="store_true",
                   help="EigenSNP workflow: also write P.eigensnp.model.tsv (per PCA SNP: alleles, mean, s.d., loadings) for "
                        "--gpca-project-model")
    p.add_argument("--gpca-project-model", default=None, metavar="MODEL",
                   help="project the samples of --bed-file onto the PCs of MODEL (a P.eigensnp.model.tsv), matched by variant ID "
                        "with allele flips handled; missing calls mean-imputed -> P.projected.pca.tsv")
    p.add_argument("--gpca-make-grm", action="store_true",
                   help="EigenSNP workflow: also write the genetic relationship matrix of the kept SNPs in GCTA's binary layout "
                        "(P.grm.bin, P.grm.N.bin, P.grm.id).  Each entry is (1/K) sum of Z_j Z_k over the K kept SNPs, missing calls at "
                        "0: the divisor is K for every pair, not GCTA's per-pair count, and GCTA's GRM formula is not claimed; "
                        "P.grm.N.bin holds the SNPs where both samples are observed")
    p.add_argument("--gpca-grm-scaling", choices=("standardized", "centred"), default="standardized",
                   help="--gpca-make-grm: Z = (g - mean) / s.d. (standardized, the matrix the PCA factorises) or g - mean (centred)")
    p.add_argument("--gpca-make-king", action="store_true",
                   help="EigenSNP workflow: also write the KING-robust kinship of every sample pair over the kept SNPs to P.kin0 "
                        "(#FID1 IID1 FID2 IID2 NSNP HETHET IBS0 KINSHIP, ID1 the earlier sample in .fam order)")
    p.add_argument("--gpca-king-table-filter", type=float, default=None, metavar="X",
                   help="--gpca-make-king: write only the pairs with kinship >= X")
    p.add_argument("--gpca-king-cutoff", type=float, default=None, metavar="X",
                   help="EigenSNP workflow: drop related samples before the PCA (0 < X < 0.5; 0.0884 = second degree).  While a pair with "
                        "KING-robust kinship > X remains, the sample with the most such partners leaves (ties: the later one in .fam "
                        "order) -> P.king.cutoff.in.id / .out.id.  The PCs are fitted on the in-set and every sample is projected onto "
                        "them; SNP QC, means and s.d. stay over all samples")
    p.add_argument("--gpca-make-pcrelate", type=int, default=None, metavar="P",
                   help="EigenSNP workflow: also write the PC-Relate kinship of every sample pair over the kept SNPs, adjusted for the first "
                        "P PCs of the scores this run writes (0 <= P <= --eigensnp-k-global, at most 32; 0 = the homogeneous estimator), to "
                        "P.pcrelate.kin (#FID1 IID1 FID2 IID2 NSNP KINSHIP, ID1 the earlier sample in .fam order) and the inbreeding "
                        "coefficients to P.pcrelate.inbreed (#FID IID NSNP F).  With --gpca-king-cutoff the regression is fitted on the "
                        "in-set, otherwise on every sample.  Needs the matrix resident on the device")
    p.add_argument("--gpca-pcrelate-maf-bound", type=float, default=None, metavar="T",
                   help="--gpca-make-pcrelate: an entry counts when its individual-specific allele frequency lies in (T, 1 - T); "
                        "0 <= T < 0.5 [default: 0.01]")
    p.add_argument("--gpca-pcrelate-table-filter", type=float, default=None, metavar="X",
                   help="--gpca-make-pcrelate: write only the pairs with kinship >= X (P.pcrelate.inbreed stays whole)")
    p.add_argument("--gpca-indep-pairwise", nargs=2, default=None, metavar=("WINDOW", "R2"),
                   help="EigenSNP workflow: prune SNPs in linkage disequilibrium before the GRM, KING and the PCA (plink's "
                        "--indep-pairwise with step 1).  WINDOW = a variant count such as 50 (each kept SNP against the next 49 of its "
                        "chromosome) or a span such as 250kb; 0 < R2 < 1.  Of a pair of kept SNPs with unphased r^2 > R2 the one with the "
                        "smaller minor-allele frequency leaves (ties: the later one) -> P.prune.in / P.prune.out.  Needs the matrix "
                        "resident on the device; plink's exact output is not claimed")
    p.add_argument("--gpca-ld-score", default=None, metavar="WINDOW",
                   help="EigenSNP workflow: after the PCA outputs, the LD score of every SNP that passes the SNP QC: L2 = 1 + the sum of "
                        "the bias-adjusted unphased r^2 with the SNPs of its chromosome at most WINDOW away on both sides (the grammar of "
                        "--gpca-indep-pairwise's WINDOW; 1000kb is the recommendation), summed on the device -> P.l2.ldscore (CHR SNP BP "
                        "L2), P.l2.M, P.l2.M_5_50.  Every sample enters, relatives and samples that fail the sample QC included.  Needs "
                        "the matrix resident on the device")
    p.add_argument("--gpca-assoc-ldsc", action="store_true",
                   help="--gpca-ld-score and --gpca-assoc-pheno: LD-score regression of every trait's scan statistics (T_STAT^2 or "
                        "Z_STAT^2) on the LD scores, 200 jackknife blocks -> P.ldsc.summary (#TRAIT TEST N M_USED MEAN_CHI2 LAMBDA_GC "
                        "INTERCEPT INTERCEPT_SE H2 H2_SE RATIO RATIO_SE).  The intercept measures confounding, H2 the SNP heritability "
                        "(of a case / control trait: on the observed scale)")
    p.add_argument("--gpca-assoc-pheno", default=None, metavar="FILE",
                   help="EigenSNP workflow: after everything else is written, test every SNP that passes the SNP QC (call rate, MAF, HWE; "
                        "the LD blocks and --gpca-indep-pairwise shape the PCA, not the test set) against every trait column of FILE "
                        "(header `FID IID name...`, NA = missing) by least squares with the PCs as covariates, a missing call imputed to "
                        "the SNP's mean -> P.<trait>.assoc.linear (#CHROM POS ID A1 OBS_CT A1_FREQ BETA SE T_STAT LOG10P).  A sample "
                        "counts when every trait and covariate is present for it and, with --gpca-king-cutoff, it is in the in-set.  "
                        "Needs the matrix resident on the device; traits + PCs + covariates <= 64")
    p.add_argument("--gpca-assoc-logistic", action="store_true",
                   help="--gpca-assoc-pheno: a trait column whose present values are exactly {0, 1} (1 = case) or {1, 2} (plink's coding, "
                        "2 = case) gets the logistic score test (the null model fitted once per trait; --gpca-assoc-spa adds "
                        "the saddle-point correction, --gpca-assoc-firth the approximate Firth correction) -> "
                        "P.<trait>.assoc.logistic (#CHROM POS ID A1 OBS_CT A1_FREQ BETA SE Z_STAT LOG10P); the other columns go "
                        "through the linear scan as without the flag.  PCs + covariates + 3 <= 64")
    p.add_argument("--gpca-assoc-spa", action="store_true",
                   help="--gpca-assoc-logistic: the saddle-point correction (SPA, as SAIGE and regenie --spa) of every test with "
                        "|Z_STAT| >= the cutoff: LOG10P then comes from the saddle-point approximation of the score's null distribution, "
                        "which a rare variant in an unbalanced trait needs, and a column SPA says Y (corrected), N (below the cutoff: the "
                        "normal value) or F (the correction did not converge: the normal value); BETA, SE and Z_STAT stay the score test's")
    p.add_argument("--gpca-assoc-spa-z", type=float, default=None, metavar="X",
                   help="--gpca-assoc-spa: the cutoff, at least 0.5, or inf for no correction [default: 2]")
    p.add_argument("--gpca-assoc-firth", action="store_true",
                   help="--gpca-assoc-logistic: the approximate Firth correction (as regenie --firth --approx) of every test with "
                        "|Z_STAT| >= the cutoff: one coefficient on the covariate-adjusted genotype by Firth's penalised likelihood, the null "
                        "model as offset.  BETA, SE and LOG10P are then Firth's (finite where every carrier is a case), Z_STAT stays the score "
                        "test's, and a column FIRTH says Y (corrected), N (below the cutoff) or F (the fit failed: the score test's values).  "
                        "Not together with --gpca-assoc-spa")
    p.add_argument("--gpca-assoc-firth-z", type=float, default=None, metavar="X",
                   help="--gpca-assoc-firth: the cutoff, at least 0, or inf for no correction [default: 1.959964]")
    p.add_argument("--gpca-assoc-set-list", default=None, metavar="FILE",
                   help="--gpca-assoc-logistic: gene-level set tests after the per-SNP scans.  FILE is regenie's set list, one set per "
                        "line: NAME CHROM POS ID1,ID2,... (IDs that the SNP QC removed are dropped).  Every case / control trait gets "
                        "P.<trait>.assoc.set (#SET CHROM POS N_VAR N_USED BURDEN_BETA BURDEN_SE BURDEN_Z BURDEN_LOG10P SKAT_Q SKAT_LOG10P "
                        "SKAT): a weighted burden test and SKAT (its p-value by Kuonen's saddle point: SKAT = Y; N = the bulk "
                        "approximation, F = the saddle point failed) from the covariance of the set's scores under the null model.  A "
                        "set with no variant left, or with more than 128, gets NA")
    p.add_argument("--gpca-assoc-set-max-maf", type=float, default=None, metavar="X",
                   help="--gpca-assoc-set-list: a listed variant enters its set when its minor-allele frequency over the included "
                        "observed calls is at most X, 0 < X <= 0.5 [default: 0.01]")
    p.add_argument("--gpca-assoc-set-weights", default=None, metavar="KIND",
                   help="--gpca-assoc-set-list: beta = Beta(maf; 1, 25) weights, flat = 1 [default: beta]")
    p.add_argument("--gpca-assoc-cc-freq", action="store_true",
                   help="--gpca-assoc-logistic: the genotype counts and A1 frequencies of every SNP among the controls and the cases "
                        "of every case / control trait, over the scan's include set -> <out>.<trait>.frq.cc (the .frq.strat format "
                        "with the groups CTRL and CASE)")
    p.add_argument("--gpca-within", default=None, metavar="FILE",
                   help="--eigensnp: the sample groups of --gpca-freq-strat and --gpca-fst, a table `FID IID GROUP` with that header; "
                        "NA = no group; at most 64 groups")
    p.add_argument("--gpca-freq-strat", action="store_true",
                   help="--gpca-within: the genotype counts, A1 frequency and HWE p-value of every SNP that passes the SNP QC inside "
                        "every group -> <out>.frq.strat")
    p.add_argument("--gpca-fst", default=None, metavar="METHOD",
                   help="--gpca-within: Fst between every pair of groups over the SNPs that pass the SNP QC, hudson (Bhatia et al. "
                        "2013) or wc (Weir and Cockerham 1984; with more than two groups also jointly) -> <out>.fst.summary")
    p.add_argument("--gpca-fst-variants", action="store_true", help="--gpca-fst: also the per-SNP terms -> <out>.fst.var")
    p.add_argument("--gpca-f2", action="store_true",
                   help="--gpca-within: the unbiased f2 of every pair of groups over the SNPs that pass the SNP QC, with its weighted "
                        "block-jackknife standard error -> <out>.f2.summary")
    p.add_argument("--gpca-fstats", default=None, metavar="FILE",
                   help="--gpca-within: the statistics FILE lists, one per line: `f2 A B`, `f3 C A B` (C is the target) or `f4 A B C D` "
                        "with group names -> <out>.fstats (estimate, jackknife SE, Z)")
    p.add_argument("--gpca-fstat-block", default=None, metavar="SPEC",
                   help="--gpca-f2 / --gpca-fstats: the jackknife blocks, a variant count such as 500 or a span such as 5000kb; a block "
                        "ends at every change of chromosome [default: 5000kb]")
    p.add_argument("--gpca-sample-missing", action="store_true",
                   help="--eigensnp: the missing calls of every sample over the SNPs that pass the SNP QC -> <out>.smiss (#FID IID "
                        "MISSING_CT OBS_CT F_MISS)")
    p.add_argument("--gpca-het", action="store_true",
                   help="--eigensnp: the observed and expected homozygous calls and the inbreeding coefficient F of every sample over "
                        "the SNPs that pass the SNP QC (plink --het, allele frequencies from all samples) -> <out>.het (#FID IID O_HOM "
                        "E_HOM OBS_CT F)")
    p.add_argument("--gpca-mind", type=float, default=None, metavar="X",
                   help="--eigensnp: drop a sample from the fit, PC-Relate's training set and the scans when more than X of its calls "
                        "are missing (0 <= X < 1) -> <out>.sampleqc.in.id / .out.id; every sample is still projected")
    p.add_argument("--gpca-het-sd", type=float, default=None, metavar="K",
                   help="--eigensnp: drop a sample whose F lies more than K standard deviations from the mean F of the samples that "
                        "pass --gpca-mind (K > 0; one round) -> <out>.sampleqc.in.id / .out.id")
    p.add_argument("--gpca-homozyg", action="store_true",
                   help="--eigensnp: runs of homozygosity of every sample over the SNPs that pass the SNP QC (plink --homozyg's sliding "
                        "window) -> <out>.hom (#FID IID CHROM SNP1 SNP2 POS1 POS2 KB NSNP DENSITY PHOM PHET) and <out>.hom.indiv (#FID IID "
                        "NSEG KB KBAVG FROH); any flag below implies it")
    p.add_argument("--gpca-homozyg-window-snp", type=int, default=None, metavar="W", help="the scanning window in SNPs (1 .. 64) [default: 50]")
    p.add_argument("--gpca-homozyg-window-het", type=int, default=None, metavar="H",
                   help="het calls a window may hold and still be a hit (0 .. W) [default: 1]")
    p.add_argument("--gpca-homozyg-window-missing", type=int, default=None, metavar="M",
                   help="missing calls a window may hold and still be a hit (0 .. W) [default: 5]")
    p.add_argument("--gpca-homozyg-window-threshold", default=None, metavar="X",
                   help="the share of hits among the windows over a SNP that puts it in a run, a decimal number in [0, 1] taken as its "
                        "exact fraction [default: 0.05]")
    p.add_argument("--gpca-homozyg-snp", type=int, default=None, metavar="N", help="SNPs a run needs at least [default: 100]")
    p.add_argument("--gpca-homozyg-kb", type=float, default=None, metavar="X", help="kb a run spans at least [default: 1000]")
    p.add_argument("--gpca-homozyg-density", type=float, default=None, metavar="X", help="kb per SNP a run holds at most [default: 50]")
    p.add_argument("--gpca-homozyg-gap", type=float, default=None, metavar="X",
                   help="a gap of more than X kb between two SNPs ends a run [default: 1000]")
    p.add_argument("--gpca-homozyg-het", type=int, default=None, metavar="N", help="het calls a run holds at most [default: no limit]")
    p.add_argument("--gpca-admixture", type=int, default=None, metavar="K",
                   help="--eigensnp: admixture proportions of every sample in K ancestral populations (1 .. 16), the ADMIXTURE model "
                        "fitted by accelerated EM over the SNPs the PCA is fitted on; samples outside the KING in-set or failing the "
                        "sample QC get proportions without shaping the frequencies -> <out>.K.Q, .Q.id, .P, .P.id and .admix.log")
    p.add_argument("--gpca-admixture-seed", type=int, default=None, metavar="S", help="the seed of the starting point [default: 0]")
    p.add_argument("--gpca-admixture-max-iter", type=int, default=None, metavar="N", help="EM steps at most [default: 2000]")
    p.add_argument("--gpca-admixture-tol", type=float, default=None, metavar="X",
                   help="stop when a cycle gains less than X times the log-likelihood [default: 1e-7]")
    p.add_argument("--gpca-admixture-no-accel", action="store_true", help="plain EM steps, without the SQUAREM acceleration")
    p.add_argument("--gpca-admixture-supervised", action="store_true",
                   help="the samples with a group in --gpca-within are references of known ancestry: K must be the number of groups, and "
                        "column k of the result is group k")
    p.add_argument("--gpca-admixture-cv", type=int, nargs="?", const=5, default=None, metavar="V",
                   help="--gpca-admixture: the V-fold cross-validation error of the fit (2 .. 64): a random V-th of the observed calls is "
                        "hidden from a refit and scored by its binomial deviance, once per fold -> <out>.admix.cv [default V: 5]")
    p.add_argument("--gpca-admixture-cv-seed", type=int, default=None, metavar="S", help="the seed of the folds [default: 0]")
    p.add_argument("--gpca-admixture-cv-k", default=None, metavar="A-B",
                   help="--gpca-admixture-cv: also score every K of A .. B (1 <= A <= B <= 16) into <out>.admix.cv, to choose K")
    p.add_argument("--gpca-assoc-pcs", type=int, default=None, metavar="P",
                   help="--gpca-assoc-pheno: the first P columns of the scores this run writes are covariates (0 <= P <= "
                        "--eigensnp-k-global) [default: every column]")
    p.add_argument("--gpca-assoc-covar", default=None, metavar="FILE",
                   help="--gpca-assoc-pheno: further covariates, a table in the format of the phenotype file")
    p.add_argument("--gpca-assoc-vif", type=float, default=None, metavar="X",
                   help="--gpca-assoc-pheno: a SNP whose variance inflation against the covariates exceeds X gets NA (plink's --vif) "
                        "[default: 50]")
    p.add_argument("--gpca-qtl-pheno", default=None, metavar="FILE",
                   help="EigenSNP workflow: after everything else is written, test every SNP that passes the SNP QC against every column "
                        "of FILE (`FID IID name...`, up to 2^20 traits: a molecular QTL or PheWAS screen) in one wide pass on the GPU, "
                        "and keep the pairs beyond the threshold in <out>.qtl.hits and the best SNP of every trait in <out>.qtl.best")
    p.add_argument("--gpca-qtl-pcs", type=int, default=None, metavar="P",
                   help="--gpca-qtl-pheno: the first P columns of the scores this run writes are covariates (0 <= P <= "
                        "--eigensnp-k-global) [default: every column]")
    p.add_argument("--gpca-qtl-covar", default=None, metavar="FILE",
                   help="--gpca-qtl-pheno: further covariates, a table in the format of the phenotype file (at most 63 with the PCs)")
    p.add_argument("--gpca-qtl-log10p", type=float, default=None, metavar="X",
                   help="--gpca-qtl-pheno: keep the pairs with -log10 p >= X [default: 5]")
    p.add_argument("--gpca-qtl-t", type=float, default=None, metavar="X", help="--gpca-qtl-pheno: keep the pairs with |t| >= X instead")
    p.add_argument("--gpca-qtl-vif", type=float, default=None, metavar="X",
                   help="--gpca-qtl-pheno: a SNP whose variance inflation against the covariates exceeds X is not tested [default: 50]")
    p.add_argument("--gpca-qtl-cis-pos", default=None, metavar="FILE",
                   help="--gpca-qtl-pheno: cis-QTL mapping after the scan: FILE is a `TRAIT CHROM POS` table; every trait with a position is "
                        "tested against the SNPs within the window around it, with a permutation null and its beta approximation, into "
                        "<out>.qtl.cis")
    p.add_argument("--gpca-qtl-cis-window", type=int, default=None, metavar="BP", help="--gpca-qtl-cis-pos: |SNP - POS| <= BP [default: 1000000]")
    p.add_argument("--gpca-qtl-cis-perm", type=int, default=None, metavar="P",
                   help="--gpca-qtl-cis-pos: permutations of the traits [default: 1000; 0 = nominal only, the beta columns are NA]")
    p.add_argument("--gpca-qtl-cis-seed", type=int, default=None, metavar="S", help="--gpca-qtl-cis-pos: the seed of the permutation table [default: 0]")
    p.add_argument("--gpca-qtl-cis-only", action="store_true", help="--gpca-qtl-cis-pos: skip the scan of every SNP against every trait")
    return p


def grm_bands(n: int, max_entries: int = 1 << 26):
    """Consecutive row bands [row0, row1) of an n-sample lower triangle, each of at most max_entries entries (at least one row)."""
    r0 = 0
    while r0 < n:
        r1 = r0 + 1
        while r1 < n and (r1 + 1) * (r1 + 2) // 2 - r0 * (r0 + 1) // 2 <= max_entries:
            r1 += 1
        yield r0, r1
        r0 = r1


def _engine_modes(a, bed_samples: int = 0):
    """(precision, storage); storage "auto": a .bed of >= 1 024 samples stays in its own 2-bit form (a quarter of the HBM, and the
    packed kernels are faster there: 7.9 vs 11.1 ms at 1M x 10k); narrower matrices and VCF input are int8 (the packed rows pad
    to 1 024 samples)."""
    from . import _lib
    if a.gpca_storage == "auto":
        a.gpca_storage = "2bit" if bed_samples >= 1024 else "int8"
    return (_lib.PREC_I8_EXACT if a.gpca_precision == "i8" else _lib.PREC_F32_MFMA,
            _lib.STORE_2BIT if a.gpca_storage == "2bit" else _lib.STORE_INT8)


def _log(msg: str):
    print(f"[genomic_pca_amd] {msg}", file=sys.stderr, flush=True)


def _ensure_parent(prefix: str):
    parent = os.path.dirname(prefix)
    if parent and not os.path.exists(parent):
        os.makedirs(parent, exist_ok=True)                                         # main.rs:372-377


def run_vcf_workflow(a) -> int:
    if not a.vcf_dir or a.components is None:
        raise SystemExit("error: --vcf-dir and --components are required unless --eigensnp is given")
    t0 = time.time()
    files = sorted(os.path.join(a.vcf_dir, f) for f in os.listdir(a.vcf_dir) if f.endswith(".vcf") or f.endswith(".vcf.gz"))
    if not files:
        raise SystemExit(f"No VCF files found in {a.vcf_dir}")                       # main.rs:153-155
    maf = 0.01 if a.maf is None else a.maf
    samples, ids, chunks = None, [], []
    for f in files:
        s, i, g = gio.read_vcf(f, maf)
        if samples is None:
            samples = s
        elif s != samples:
            raise SystemExit(f"Sample mismatch between VCF files: {f}")             # vcf.rs:78-95
        ids += i
        chunks.append(g)
    G = np.concatenate(chunks, axis=0) if chunks else np.zeros((0, 0), np.int8)
    _log(f"{len(files)} VCF files, {G.shape[0]} variants x {len(samples or [])} samples in {time.time() - t0:.2f}s")
    if G.shape[0] == 0:
        raise SystemExit("No variants available to build matrix.")                  # vcf.rs:321-323
    prec, store = _engine_modes(a)
    model = PCA(device=a.device, precision=prec, storage=store)
    model.rfit(G.T, a.components, 10, a.rfit_seed, None, power_iters=a.gpca_rfit_power_iters)                            # main.rs:636-656 (x = samples x variants)
    pcs = model.transform()
    _ensure_parent(a.output_prefix)
    gio.write_principal_components(a.output_prefix, "vcf.pca.tsv", samples, pcs)    # main.rs:231
    gio.write_eigenvalues(a.output_prefix, model.explained_variance() if a.write_eigenvalues else [])   # main.rs:232, 676
    _log(f"VCF workflow done in {time.time() - t0:.2f}s")
    return 0


def _load_bed(eng, a, fs, cols) -> bool:
    """The .bed payload into the engine: resident (decoded on the GPU from 256 MiB row chunks of the memory map), or -- when
    it does not fit the device, or on request -- out of core: every pass walks the memory map panel by panel through a ring
    of HBM buffers, and the HBM that is left keeps the leading panels (gpca_stream_set_cache).  The reference's solver pulls
    strips through the accessor on every pass in the same way (prepare.rs:1839-2022, main.rs:322).  Returns True when the matrix is
    walked out of core."""
    from . import _lib
    from .engine import PanelSource
    rows = fs.bed_rows
    lut = np.array([2, -127, 1, 0], np.int8)                                         # count_a1 (prepare.rs:622-629)
    shift = None if cols is None else (2 * (cols % 4)).astype(np.uint8)

    def subset(r0, n):                                                               # kept sample columns of rows [r0, r0 + n)
        return lut[(np.asarray(rows[r0:r0 + n])[:, cols // 4] >> shift) & 3]
    n_samples = fs.n_samples if cols is None else len(cols)
    if a.gpca_stream == "auto":
        # resident needs the matrix (1 B or 0.25 B per genotype, rows padded) plus the solver's workspace (gpca.h,
        # gpca_get_device_memory): a load that fits with nothing to spare would only fail later, in gpca_rsvd
        free, _ = eng.device_memory()
        free = int(os.environ.get("GPCA_CLI_FREE_BYTES", free))       # (test hook: pretend the device is smaller)
        per_row = -(-n_samples // 1024) * 1024 // (4 if a.gpca_storage == "2bit" else 1) + 512
        need = rows.shape[0] * (per_row + 1024) + n_samples * 8192 + (1 << 30)
        if need > free:
            _log(f"the genotype matrix needs about {need / 2**30:.1f} GiB resident, {free / 2**30:.1f} GiB are free: walking it out of core")
            a.gpca_stream = "on"
    if a.gpca_stream != "on":
        try:
            if cols is None:
                eng.upload_bed2bit(rows, fs.n_samples)
            else:
                eng.load_from_source(PanelSource.host_i8(subset), rows.shape[0], n_samples)
            return False
        except _lib.GpcaError as e:
            if a.gpca_stream == "off" or e.status != _lib.GPCA_ERR_OOM:
                raise
            _log("the genotype matrix does not fit the device: walking it out of core")
    # the memory-mapped payload itself is the source (GPCA_PANEL_MAPPED_BED): the library's copy threads stage its panels, no callback
    src = PanelSource.mapped_bed(rows) if cols is None else PanelSource.host_i8(subset)
    eng.stream_open(src, rows.shape[0], n_samples, panel_rows=a.gpca_panel_rows, cache_bytes=-1)
    return True


def run_eigensnp_workflow(a) -> int:
    if not a.bed_file or not a.ld_block_file:
        raise SystemExit("error: --bed-file and --ld-block-file are required when --eigensnp is used")   # main.rs:296-301
    t0 = time.time()
    fs = gio.read_plink(a.bed_file)
    prec, store = _engine_modes(a, fs.n_samples)
    eng = GpcaEngine(device=a.device, precision=prec, storage=store)
    sample_ids = fs.sample_ids
    cols = None
    if a.eigensnp_sample_keep_file:                                                  # prepare.rs:1058-1096
        keep_ids = set(gio.read_sample_keep_file(a.eigensnp_sample_keep_file))
        cols = np.array([i for i, s in enumerate(fs.sample_ids) if s in keep_ids], np.int64)
        if len(cols) == 0:
            _log("No samples available after sample QC."); return 0
        sample_ids = [fs.sample_ids[i] for i in cols]
    streamed = _load_bed(eng, a, fs, cols)
    if streamed and a.gpca_make_pcrelate is not None:
        raise SystemExit(PCRELATE_NEEDS_RESIDENT)
    if streamed and a.gpca_assoc_pheno is not None:
        raise SystemExit(ASSOC_NEEDS_RESIDENT)
    if streamed and a.gpca_qtl_pheno is not None:
        raise SystemExit(QTL_NEEDS_RESIDENT)
    if streamed and a.gpca_within is not None and _strat_asked(a):
        raise SystemExit(STRAT_NEEDS_RESIDENT)
    if streamed and _sample_qc_asked(a):
        raise SystemExit(SAMPLE_QC_NEEDS_RESIDENT)
    if streamed and _homozyg_asked(a):
        raise SystemExit(HOMOZYG_NEEDS_RESIDENT)
    if streamed and a.gpca_ld_score is not None:
        raise SystemExit(LD_SCORE_NEEDS_RESIDENT)
    if streamed and a.gpca_admixture is not None:
        raise SystemExit(ADMIX_NEEDS_RESIDENT)
    st = eng.snp_stats(QcConfig(a.eigensnp_min_call_rate, a.eigensnp_min_maf, a.eigensnp_max_hwe_p))
    qc_pass = None
    if _sample_qc_asked(a) and len(sample_ids) and int(st["keep"].sum()):
        qc_pass = _sample_qc(eng, a, fs, cols, sample_ids, st)
    if _homozyg_asked(a) and len(sample_ids) and int(st["keep"].sum()):
        _homozyg(eng, a, fs, cols, sample_ids, st)
    blocks = gio.parse_ld_block_file(a.ld_block_file)
    keep, by_tag = gio.map_snps_to_ld_blocks(blocks, fs.chromosomes, fs.positions, st["keep"])
    _log(f"{int(st['keep'].sum())} / {len(st['keep'])} SNPs passed QC; {int(keep.sum())} fall in {len(by_tag)} LD blocks")
    if len(sample_ids) == 0 or int(keep.sum()) == 0:
        _log("No samples or SNPs available for EigenSNP PCA after preparation.")     # main.rs:349-352
        return 0
    eng.set_standardization(st["mu"], st["sigma"], keep)
    if a.gpca_indep_pairwise:
        keep, by_tag = _indep_pairwise(eng, a, fs, st, keep, by_tag)
    if a.gpca_make_grm:
        _ensure_parent(a.output_prefix)
        fids = fs.family_ids if cols is None else [fs.family_ids[i] for i in cols]
        gio.write_grm(a.output_prefix, fids, sample_ids,
                      (eng.grm(a.gpca_grm_scaling, rows=b, npairs=True) for b in grm_bands(len(sample_ids))))
        _log(f"GRM of {len(sample_ids)} samples over {int(keep.sum())} SNPs written to {a.output_prefix}.grm.bin")
    inset = None
    if a.gpca_make_king or a.gpca_king_cutoff is not None:
        inset = _king(eng, a, fs, cols, sample_ids, int(keep.sum()), qc_pass)
    if qc_pass is not None:                                                          # the in-set is KING's and the sample QC's
        inset = qc_pass.copy() if inset is None else (np.asarray(inset, bool) & qc_pass)
        if int(inset.sum()) < 2:
            raise SystemExit("error: --gpca-mind / --gpca-het-sd leave fewer than 2 samples to fit the PCA on")
    acc = MicroarrayGenotypeAccessor(eng)
    rows = acc.original_indices_of_pca_snps()
    row_to_id = {int(r): i for i, r in enumerate(rows)}
    specs = [LdBlockSpecification(tag, [row_to_id[r] for r in rs]) for tag, rs in by_tag]
    cfg = EigenSNPCoreAlgorithmConfig(
        target_num_global_pcs=a.eigensnp_k_global, components_per_ld_block=a.eigensnp_components_per_block,
        subset_factor_for_local_basis_learning=a.eigensnp_subset_factor,
        min_subset_size_for_local_basis_learning=a.eigensnp_min_subset_size,
        max_subset_size_for_local_basis_learning=a.eigensnp_max_subset_size,
        global_pca_sketch_oversampling=a.eigensnp_global_oversampling,
        global_pca_num_power_iterations=a.eigensnp_global_power_iter,
        local_rsvd_sketch_oversampling=a.eigensnp_local_oversampling,
        local_rsvd_num_power_iterations=a.eigensnp_local_power_iter, random_seed=a.eigensnp_seed,
        snp_processing_strip_size=a.eigensnp_snp_strip_size, refine_pass_count=a.eigensnp_refine_passes,
        collect_diagnostics=a.eigensnp_collect_diagnostics)
    n_fit = len(sample_ids) if inset is None else int(inset.sum())
    k = min(cfg.target_num_global_pcs, n_fit, len(rows))
    cfg.target_num_global_pcs = k
    cfg.global_pca_sketch_oversampling = max(0, min(cfg.global_pca_sketch_oversampling, min(n_fit, len(rows)) - k))
    if a.gpca_make_pcrelate is not None and a.gpca_make_pcrelate > k:
        raise SystemExit(f"error: --gpca-make-pcrelate {a.gpca_make_pcrelate} asks for more PCs than the {k} this run computes")
    if a.gpca_assoc_pcs is not None and a.gpca_assoc_pcs > k:
        raise SystemExit(f"error: --gpca-assoc-pcs {a.gpca_assoc_pcs} asks for more PCs than the {k} this run computes")
    if a.gpca_qtl_pcs is not None and a.gpca_qtl_pcs > k:
        raise SystemExit(f"error: --gpca-qtl-pcs {a.gpca_qtl_pcs} asks for more PCs than the {k} this run computes")
    if inset is not None and not inset.all():
        eng.set_sample_mask(inset.astype(np.uint8))                                # the fit sees the in-set only
    out, _ = EigenSNPCoreAlgorithm(cfg).compute_pca(acc, specs, local_stage=a.gpca_eigensnp_local_stage, project_all=inset is not None)
    # with the cutoff: every sample projected onto the in-set's fit, the relatives included
    scores = out.final_sample_principal_component_scores if inset is None else out.projected_sample_scores
    _ensure_parent(a.output_prefix)
    gio.write_principal_components(a.output_prefix, "eigensnp.pca.tsv", sample_ids, scores)
    gio.write_eigenvalues(a.output_prefix, out.final_principal_component_eigenvalues)
    gio.write_loadings(a.output_prefix, [fs.variant_ids[r] for r in rows], [fs.chromosomes[r] for r in rows],
                       [int(fs.positions[r]) for r in rows], out.final_snp_principal_component_loadings)
    if a.gpca_save_model:
        stz = eng.get_standardization()
        gio.write_model(a.output_prefix, gio.ProjectionModel(
            [fs.variant_ids[r] for r in rows], [fs.chromosomes[r] for r in rows], [int(fs.positions[r]) for r in rows],
            [fs.allele1[r] for r in rows], [fs.allele2[r] for r in rows], stz["mu"][rows], stz["sigma"][rows],
            np.asarray(out.final_snp_principal_component_loadings, np.float32), np.asarray(out.final_principal_component_eigenvalues, np.float64),
            n_fit))
    if a.gpca_admixture is not None:                                                 # while the handle carries the PCA's keep mask
        _admix(eng, a, fs, cols, sample_ids, rows, inset)
    if a.gpca_make_pcrelate is not None:
        _pcrelate(eng, a, fs, cols, sample_ids, np.asarray(scores, np.float64)[:, :a.gpca_make_pcrelate], inset, len(rows))
    if a.gpca_within is not None and _strat_asked(a):
        _strat(eng, a, fs, cols, sample_ids, st)
    l2 = _ld_score(eng, a, fs, st) if a.gpca_ld_score is not None else None
    if a.gpca_assoc_pheno is not None:
        _assoc(eng, a, fs, cols, sample_ids, np.asarray(scores, np.float64), inset, st, l2)
    if a.gpca_qtl_pheno is not None:
        _qtl(eng, a, fs, cols, sample_ids, np.asarray(scores, np.float64), inset, st)
    eng.close()
    _log(f"EigenSNP workflow done in {time.time() - t0:.2f}s")
    return 0


ADMIX_NEEDS_RESIDENT = ("error: --gpca-admixture needs the genotype matrix resident on the device: the fit of a matrix walked out of core "
                        "is not implemented")


def _admix(eng, a, fs, cols, sample_ids, rows, inset):
    """--gpca-admixture K: the admixture fit (gpca_admix) over the rows the PCA was fitted on (the handle's keep mask as the PCA left
    it: after the LD-block mapping and --gpca-indep-pairwise) and every sample: mode 0 inside the in-set of --gpca-king-cutoff and the
    sample QC, mode 2 outside it, mode 1 for a sample with a group under --gpca-admixture-supervised.  Writes P.K.Q, .Q.id, .P, .P.id
    and .admix.log with the columns in io.admix_order."""
    from . import _lib
    fids = fs.family_ids if cols is None else [fs.family_ids[i] for i in cols]
    K, n = a.gpca_admixture, len(sample_ids)
    seed = 0 if a.gpca_admixture_seed is None else a.gpca_admixture_seed
    kw = dict(seed=seed, max_iter=2000 if a.gpca_admixture_max_iter is None else a.gpca_admixture_max_iter,
              tol=1e-7 if a.gpca_admixture_tol is None else a.gpca_admixture_tol, accel=not a.gpca_admixture_no_accel)
    mode = np.zeros(n, np.uint8) if inset is None else np.where(np.asarray(inset, bool), 0, 2).astype(np.uint8)
    try:
        if a.gpca_admixture_supervised:
            labels, _names = gio.align_within(a.gpca_within_table, fids, sample_ids)
            Q0, F0 = eng.admix_init(K, seed)
            Q0, fixed = gio.admix_supervised(labels, K, Q0)
            mode[fixed == 1] = 1                                                     # a labelled sample is a reference wherever it stands
            r = eng.admix(K, mode=mode, Q=Q0, F=F0, **kw)
        else:
            r = eng.admix(K, mode=mode, **kw)
    except _lib.GpcaError as e:
        if e.status == _lib.GPCA_ERR_STATE:
            raise SystemExit(ADMIX_NEEDS_RESIDENT) from None
        raise
    order = gio.admix_order(r["Q"], mode)
    _ensure_parent(a.output_prefix)
    gio.write_admix(a.output_prefix, K, fids, sample_ids, [fs.variant_ids[i] for i in rows], r["Q"][:, order], r["F"][:, order],
                    dict(seed=seed, steps=r["steps"], cycles=r["cycles"], converged=r["converged"], loglik=r["loglik"]))
    _log(f"admixture (K = {K}) of {n} samples ({int((mode == 1).sum())} references, {int((mode == 2).sum())} projected) over {len(rows)} SNPs: "
         f"{r['steps']} steps, {'converged' if r['converged'] else 'not converged'}, log-likelihood {r['loglik']:.4f}, written to "
         f"{a.output_prefix}.{K}.Q")
    if a.gpca_admixture_cv_ks is not None:
        # --gpca-admixture-cv: the same mode bytes, seed, max-iter, tol and accel, and the supervised fit's start; every K of the range
        folds, cv_seed = a.gpca_admixture_cv, 0 if a.gpca_admixture_cv_seed is None else a.gpca_admixture_cv_seed
        table = []
        for k in a.gpca_admixture_cv_ks:
            cv = eng.admix_cv(k, folds=folds, cv_seed=cv_seed, mode=mode, **(dict(Q=Q0, F=F0) if a.gpca_admixture_supervised else {}), **kw)
            table += [dict(K=k, folds=folds, cv_seed=cv_seed, fold=c, **f) for c, f in enumerate(cv["folds"])]
            _log(f"CV error (K={k}): {'NA' if cv['cv_error'] != cv['cv_error'] else '%.6f' % cv['cv_error']}")
        gio.write_admix_cv(a.output_prefix, table)
        _log(f"admixture cross-validation ({folds} folds, seed {cv_seed}) of K = {', '.join(str(k) for k in a.gpca_admixture_cv_ks)} written "
             f"to {a.output_prefix}.admix.cv")


LD_SCORE_NEEDS_RESIDENT = ("error: --gpca-ld-score needs the genotype matrix resident on the device: with the matrix walked out of core a "
                           "window crosses the panels, and the halo of rows that needs is not implemented")


def _ld_score(eng, a, fs, st):
    """--gpca-ld-score WINDOW: the LD scores (gpca_ld_score, in the row bands of io.ld_bands, always unbiased; the bands added up by
    io.ld_score_sum) of every SNP that passes the SNP QC, over every sample, into P.l2.ldscore, P.l2.M and P.l2.M_5_50.  Sets the keep
    mask to the QC mask (mu, sigma unchanged), which ends the fit's validity.  Returns L2 [K]."""
    from . import _lib
    eng.set_standardization(st["mu"], st["sigma"], st["keep"])                       # every SNP that passes the SNP QC
    rows = np.flatnonzero(st["keep"])
    K = len(rows)
    try:
        win_end = gio.ld_windows([fs.chromosomes[r] for r in rows], np.asarray(fs.positions, np.int64)[rows], a.gpca_ld_score)
    except ValueError as e:
        raise SystemExit(f"error: --gpca-ld-score: {e} (variant indices count the SNPs that pass the SNP QC)") from None

    def bands():
        for r0, r1, wm in gio.ld_bands(win_end):
            o = eng.ld_score(win_end[r0:r1], wmax=wm, rows=(r0, r1), unbiased=True, partners=True)
            yield (r0, r1), o["score"], o["partners"]
    try:
        acc, part = gio.ld_score_sum(K, bands())
    except _lib.GpcaError as e:
        if e.status == _lib.GPCA_ERR_STATE:
            raise SystemExit(LD_SCORE_NEEDS_RESIDENT) from None
        raise
    l2 = GpcaEngine.ld_score_total(acc)
    counts = eng.snp_qc_detail()[0][rows]
    maf = gio.maf_from_qc_detail(counts[:, 0], counts[:, 2], counts[:, 3])
    _ensure_parent(a.output_prefix)
    gio.write_ldscore(a.output_prefix, [fs.chromosomes[r] for r in rows], [fs.variant_ids[r] for r in rows],
                      [int(fs.positions[r]) for r in rows], l2, maf)
    mean_l2 = sum(l2.tolist()) / K if K else float("nan")
    mean_p = int(part.sum()) / K if K else float("nan")
    _log(f"LD scores (window {a.gpca_ld_score}) of {K} SNPs over {eng.dims()[1]} samples: mean L2 {mean_l2:.6g}, mean partners "
         f"{mean_p:.6g}, written to {a.output_prefix}.l2.ldscore")
    return l2


SAMPLE_QC_NEEDS_RESIDENT = ("error: --gpca-sample-missing, --gpca-het, --gpca-mind and --gpca-het-sd need the genotype matrix resident on "
                            "the device: the per-sample counts of a matrix walked out of core are not implemented")


def _sample_qc_asked(a) -> bool:
    return bool(a.gpca_sample_missing or a.gpca_het or a.gpca_mind is not None or a.gpca_het_sd is not None)


def _sample_qc(eng, a, fs, cols, sample_ids, st):
    """--gpca-sample-missing / --gpca-het / --gpca-mind / --gpca-het-sd: the per-sample counts (gpca_sample_counts, in row bands) over
    every SNP that passes the SNP QC, with the rows' weights from the QC counts of all samples (gpca_het_weights), into P.smiss and
    P.het; with a filter, the pass mask (io.sample_qc_pass) and P.sampleqc.in.id / .out.id.  Sets the keep mask to the QC mask (mu,
    sigma unchanged); the caller sets its own afterwards.  Returns the pass mask (bool [N]), or None without a filter."""
    from . import _lib
    fids = fs.family_ids if cols is None else [fs.family_ids[i] for i in cols]
    n = len(sample_ids)
    eng.set_standardization(st["mu"], st["sigma"], st["keep"])                       # every SNP that passes the SNP QC
    rows = np.flatnonzero(st["keep"])
    K = len(rows)
    need_het = a.gpca_het or a.gpca_het_sd is not None
    q = GpcaEngine.het_weights(eng.snp_qc_detail()[0][rows]) if need_het else None
    counts, qsum = np.zeros((n, 3), np.uint32), np.zeros(n, np.uint64)
    try:
        for r0, r1 in gio.sample_count_bands(K):
            r = eng.sample_counts(None if q is None else q[r0:r1], rows=(r0, r1))
            counts += r["counts"]
            if q is not None:
                qsum += r["qsum"]
    except _lib.GpcaError as e:
        if e.status == _lib.GPCA_ERR_STATE:
            raise SystemExit(SAMPLE_QC_NEEDS_RESIDENT) from None
        raise
    het = GpcaEngine.sample_het(counts, qsum) if need_het else None
    _ensure_parent(a.output_prefix)
    if a.gpca_sample_missing:
        gio.write_smiss(a.output_prefix, fids, sample_ids, counts, K)
        _log(f"missing calls of {n} samples over {K} SNPs written to {a.output_prefix}.smiss")
    if a.gpca_het:
        gio.write_het(a.output_prefix, fids, sample_ids, counts, het)
        _log(f"heterozygosity of {n} samples over {K} SNPs written to {a.output_prefix}.het")
    if a.gpca_mind is None and a.gpca_het_sd is None:
        return None
    ok, reason = gio.sample_qc_pass(counts, K, None if het is None else het[:, 2], a.gpca_mind, a.gpca_het_sd)
    gio.write_sample_qc_ids(a.output_prefix, fids, sample_ids, ok, reason)
    _log(f"sample QC: {reason.count('MIND')} samples fail --gpca-mind, {reason.count('HET')} fail --gpca-het-sd, {int(ok.sum())} of {n} pass")
    return ok.astype(bool)


HOMOZYG_NEEDS_RESIDENT = ("error: --gpca-homozyg needs the genotype matrix resident on the device: the runs of homozygosity of a matrix "
                          "walked out of core are not implemented")
HOMOZYG_VALUE_FLAGS = ("window_snp", "window_het", "window_missing", "window_threshold", "snp", "kb", "density", "gap", "het")


def _homozyg_asked(a) -> bool:
    return bool(a.gpca_homozyg or any(getattr(a, "gpca_homozyg_" + f) is not None for f in HOMOZYG_VALUE_FLAGS))


def _kb_to_bp(kb: float) -> int:
    """kb on the command line -> bp: x 1000 rounded half up (genomic_pca.cpp: kb_to_bp)"""
    return int(math.floor(float(kb) * 1000.0 + 0.5))


def _homozyg_params(a) -> dict:
    """The values of --gpca-homozyg* with their defaults, checked before anything is read; the threshold as (num, den)."""
    import re
    from fractions import Fraction
    W = 50 if a.gpca_homozyg_window_snp is None else a.gpca_homozyg_window_snp
    H = 1 if a.gpca_homozyg_window_het is None else a.gpca_homozyg_window_het
    Mi = 5 if a.gpca_homozyg_window_missing is None else a.gpca_homozyg_window_missing
    if not 1 <= W <= 64:
        raise SystemExit("error: --gpca-homozyg-window-snp must lie in [1, 64]")
    if not (0 <= H <= W and 0 <= Mi <= W):
        raise SystemExit("error: --gpca-homozyg-window-het and --gpca-homozyg-window-missing must lie in [0, --gpca-homozyg-window-snp]")
    text = "0.05" if a.gpca_homozyg_window_threshold is None else a.gpca_homozyg_window_threshold
    fr = Fraction(text) if re.fullmatch(r"[0-9]*\.?[0-9]*", text) and re.search(r"[0-9]", text) else None
    if fr is None or fr > 1 or fr.denominator > 1 << 20:
        raise SystemExit("error: --gpca-homozyg-window-threshold must be a decimal number in [0, 1] whose exact fraction has a denominator of "
                         "at most 2^20")
    snp = 100 if a.gpca_homozyg_snp is None else a.gpca_homozyg_snp
    if not 1 <= snp < 1 << 31:
        raise SystemExit("error: --gpca-homozyg-snp must lie in [1, 2^31)")
    kb = 1000.0 if a.gpca_homozyg_kb is None else a.gpca_homozyg_kb
    density = 50.0 if a.gpca_homozyg_density is None else a.gpca_homozyg_density
    gap = 1000.0 if a.gpca_homozyg_gap is None else a.gpca_homozyg_gap
    if not all(0.0 <= v <= 1e12 for v in (kb, density, gap)):
        raise SystemExit("error: --gpca-homozyg-kb, --gpca-homozyg-density and --gpca-homozyg-gap must lie in [0, 1e12]")
    if a.gpca_homozyg_het is not None and not 0 <= a.gpca_homozyg_het < 1 << 31:
        raise SystemExit("error: --gpca-homozyg-het must lie in [0, 2^31)")
    return dict(window_snp=W, window_het=H, window_missing=Mi, window_threshold=(fr.numerator, fr.denominator), min_snp=snp,
                max_het=a.gpca_homozyg_het, min_bp=_kb_to_bp(kb), max_bp_per_snp=_kb_to_bp(density), max_gap_bp=_kb_to_bp(gap))


def _homozyg(eng, a, fs, cols, sample_ids, st):
    """--gpca-homozyg: the runs of homozygosity (gpca_roh, in bands cut at chromosome starts) of every sample over every SNP that
    passes the SNP QC, the length and density rule on the records (gpca_roh_select), P.hom and P.hom.indiv.  Sets the keep mask to the
    QC mask (mu, sigma unchanged); the caller sets its own afterwards."""
    from . import _lib
    par = dict(a.gpca_homozyg_params)
    fids = fs.family_ids if cols is None else [fs.family_ids[i] for i in cols]
    eng.set_standardization(st["mu"], st["sigma"], st["keep"])                       # every SNP that passes the SNP QC
    rows = np.flatnonzero(st["keep"])
    chroms = [fs.chromosomes[r] for r in rows]
    ids = [fs.variant_ids[r] for r in rows]
    pos = np.asarray([int(fs.positions[r]) for r in rows], np.int64)
    brk = gio.roh_breaks(chroms, pos, par.pop("max_gap_bp"))
    min_bp, max_bp_per_snp = par.pop("min_bp"), par.pop("max_bp_per_snp")
    parts = []
    try:
        for r0, r1 in gio.roh_bands(brk):
            parts.append(eng.roh(brk[r0:r1], rows=(r0, r1), **par)[0])
    except _lib.GpcaError as e:
        if e.status == _lib.GPCA_ERR_STATE:
            raise SystemExit(HOMOZYG_NEEDS_RESIDENT) from None
        raise
    segs = np.concatenate(parts) if parts else np.zeros((0, 5), np.uint32)
    segs = segs[np.argsort(segs[:, 0], kind="stable")]                               # ascending (sample, first): the bands are disjoint in rows
    keep = GpcaEngine.roh_select(segs, pos, min_bp, max_bp_per_snp)
    _ensure_parent(a.output_prefix)
    gio.write_hom(a.output_prefix, fids, sample_ids, chroms, ids, pos, segs, keep, brk)
    _log(f"runs of homozygosity of {len(sample_ids)} samples over {len(rows)} SNPs: {int(keep.sum())} of {len(segs)} runs pass the length "
         f"and density rule, written to {a.output_prefix}.hom")


def _king(eng, a, fs, cols, sample_ids, n_snps, qc_pass=None):
    """--gpca-make-king / --gpca-king-cutoff: one pass over the bands of the kinship triangle (gpca_king) that writes P.kin0 and / or
    collects the pairs above the cutoff; with the cutoff, the greedy in-set (io.king_unrelated) and its id files.  qc_pass: the sample
    QC's pass mask; a related pair that touches a failed sample is dropped before the greedy rule, so that a failed sample never evicts
    a relative (the KING id files then hold the rule's verdict on the pairs that are left).  Returns the in-set mask, or None without
    the cutoff."""
    _ensure_parent(a.output_prefix)
    fids = fs.family_ids if cols is None else [fs.family_ids[i] for i in cols]
    n = len(sample_ids)
    related = []

    def bands():
        for b in gio.king_bands(n):
            kin, cnt = eng.king(rows=b, counts=True)
            if a.gpca_king_cutoff is not None:
                j, k = gio.band_pairs(*b)
                hit = np.flatnonzero(kin > a.gpca_king_cutoff)
                related.extend(zip(k[hit].tolist(), j[hit].tolist()))
            yield b, kin, cnt
    if a.gpca_make_king:
        gio.write_kin0(a.output_prefix, fids, sample_ids, bands(), a.gpca_king_table_filter)
        _log(f"KING-robust kinship of {n} samples over {n_snps} SNPs written to {a.output_prefix}.kin0")
    else:
        for _ in bands():
            pass
    if a.gpca_king_cutoff is None:
        return None
    if qc_pass is not None:
        related = [(k, j) for k, j in related if qc_pass[k] and qc_pass[j]]
    inset = gio.king_unrelated(n, related)
    gio.write_king_cutoff_ids(a.output_prefix, fids, sample_ids, inset)
    _log(f"KING cutoff {a.gpca_king_cutoff:g}: {len(related)} related pairs, {n - int(inset.sum())} of {n} samples left out of the fit")
    if int(inset.sum()) < 2:
        raise SystemExit("error: --gpca-king-cutoff leaves fewer than 2 samples to fit the PCA on")
    return inset


PCRELATE_NEEDS_RESIDENT = ("error: --gpca-make-pcrelate needs the genotype matrix resident on the device: the f32 sums are not "
                           "associative across the panels of a matrix walked out of core")


def _pcrelate(eng, a, fs, cols, sample_ids, V, inset, n_snps):
    """--gpca-make-pcrelate P: the bands of the PC-Relate triangle (gpca_pcrelate) into P.pcrelate.kin / P.pcrelate.inbreed.  V = the
    first P columns of the scores the run wrote; the regression is fitted on the KING in-set when there is one, else on everyone."""
    from . import _lib
    fids = fs.family_ids if cols is None else [fs.family_ids[i] for i in cols]
    n = len(sample_ids)
    tau = 0.01 if a.gpca_pcrelate_maf_bound is None else a.gpca_pcrelate_maf_bound
    train = None if inset is None else np.asarray(inset, bool)

    def bands():
        for b in gio.pcrelate_bands(n):
            kin, cnt = eng.pcrelate(V, train, tau, rows=b, nsnp=True)
            yield b, kin, cnt
    try:
        gio.write_pcrelate(a.output_prefix, fids, sample_ids, bands(), a.gpca_pcrelate_table_filter)
    except _lib.GpcaError as e:
        if e.status == _lib.GPCA_ERR_STATE:
            raise SystemExit(PCRELATE_NEEDS_RESIDENT) from None
        raise
    _log(f"PC-Relate kinship of {n} samples over {n_snps} SNPs, adjusted for {V.shape[1]} PCs, written to {a.output_prefix}.pcrelate.kin")


STRAT_NEEDS_RESIDENT = ("error: --gpca-within needs the genotype matrix resident on the device: the counts of a matrix walked out of core "
                        "are not implemented")


def _fstat_asked(a):
    return a.gpca_f2 or a.gpca_fstats is not None


def _strat_asked(a):
    return a.gpca_freq_strat or a.gpca_fst is not None or _fstat_asked(a)


def _within_table(a):
    """The table of --gpca-within, read once before any work on the device; refuses more than 64 groups, and fewer than 2 for --gpca-fst."""
    try:
        t = gio.read_within(a.gpca_within)
    except OSError:
        raise SystemExit(f"error: --gpca-within: cannot open {a.gpca_within}") from None
    except ValueError as e:
        raise SystemExit(f"error: --gpca-within: {e}") from None
    if len(t.names) > gio.GROUPS_MAX:
        raise SystemExit(f"error: --gpca-within: {len(t.names)} groups are more than {gio.GROUPS_MAX}")
    if a.gpca_fst is not None and len(t.names) < 2:
        raise SystemExit(f"error: --gpca-fst needs at least two groups, --gpca-within names {len(t.names)}")
    if _fstat_asked(a) and len(t.names) < 2:
        raise SystemExit(f"error: --gpca-f2 and --gpca-fstats need at least two groups, --gpca-within names {len(t.names)}")
    if len(t.names) < 1:
        raise SystemExit("error: --gpca-within names no group")
    a.gpca_fstats_list = None
    if a.gpca_fstats is not None:
        try:
            a.gpca_fstats_list = gio.read_fstats_list(a.gpca_fstats, t.names)
        except OSError:
            raise SystemExit(f"error: --gpca-fstats: cannot open {a.gpca_fstats}") from None
        except ValueError as e:
            raise SystemExit(f"error: --gpca-fstats: {e}") from None
    return t


def _snp_meta(fs, rr):
    return ([fs.chromosomes[i] for i in rr], [int(fs.positions[i]) for i in rr], [fs.variant_ids[i] for i in rr], [fs.allele1[i] for i in rr])


def _strat(eng, a, fs, cols, sample_ids, st):
    """--gpca-freq-strat / --gpca-fst: the genotype counts of every SNP that passes the SNP QC inside every group of --gpca-within
    (gpca_group_counts), in row bands, into P.frq.strat, and Fst from them (gpca_fst_hudson / gpca_fst_wc) into P.fst.summary and
    P.fst.var.  Resets the keep mask to the QC mask (mu, sigma unchanged), which ends the fit's validity; every kept sample with a
    group counts, the KING in-set or not.  --gpca-f2 / --gpca-fstats: the same bands through gpca_f2_blocks, whose counts serve the files
    above, the blocks from io.fstat_blocks over the same SNPs; gpca_fstat turns the summed blocks into P.f2.summary and P.fstats."""
    from . import _lib
    fids = fs.family_ids if cols is None else [fs.family_ids[i] for i in cols]
    labels, names = gio.align_within(a.gpca_within_table, fids, sample_ids)
    P = len(names)
    eng.set_standardization(st["mu"], st["sigma"], st["keep"])                       # every SNP that passes the SNP QC
    rows = np.flatnonzero(st["keep"])
    pairs = gio.fst_pairs(P)
    hud, wcp, wcj = np.zeros((max(len(pairs), 1), 3)), np.zeros((max(len(pairs), 1), 3)), np.zeros(3)
    fstat, need_counts = _fstat_asked(a), a.gpca_freq_strat or a.gpca_fst is not None
    if fstat:
        spec = a.gpca_fstat_block if a.gpca_fstat_block is not None else gio.FSTAT_BLOCK_DEFAULT
        block, B = gio.fstat_blocks([fs.chromosomes[i] for i in rows], [int(fs.positions[i]) for i in rows], spec)
        facc, fcnt = np.zeros((max(B, 1), len(pairs)), np.int64), np.zeros((max(B, 1), len(pairs)), np.int64)
    try:
        for bi, (r0, r1) in enumerate(gio.group_count_bands(len(rows), P, max_rows=gio.F2_BAND_ROWS_MAX if fstat else None)):
            if fstat:
                res = eng.f2_blocks(labels, block[r0:r1], P, B, rows=(r0, r1), counts=need_counts)
                facc += res[0]; fcnt += res[1]
                c = res[2] if need_counts else None
            else:
                c = eng.group_counts(labels, P, rows=(r0, r1))
            meta = _snp_meta(fs, rows[r0:r1])
            if a.gpca_freq_strat:
                gio.write_frq_strat(f"{a.output_prefix}.frq.strat", *meta, names, c, append=bi > 0)
            if a.gpca_fst == "hudson":
                res = GpcaEngine.fst_hudson(c, sums=hud, per_variant=a.gpca_fst_variants)
                if a.gpca_fst_variants:
                    gio.write_fst_var(a.output_prefix, "hudson", *meta[:3], names, np.stack([res[2], res[3]], -1), append=bi > 0)
            elif a.gpca_fst == "wc":
                abc = np.zeros((r1 - r0, len(pairs), 3))
                for q, (j, i) in enumerate(pairs):                                   # r = 2 on each pair
                    use = np.zeros(P, np.uint8); use[[j, i]] = 1
                    res = GpcaEngine.fst_wc(c, use, sums=wcp[q], per_variant=a.gpca_fst_variants)
                    if a.gpca_fst_variants:
                        abc[:, q] = res[2]
                if P > 2:
                    GpcaEngine.fst_wc(c, None, sums=wcj)
                if a.gpca_fst_variants:
                    gio.write_fst_var(a.output_prefix, "wc", *meta[:3], names, abc, append=bi > 0)
    except _lib.GpcaError as e:
        if e.status == _lib.GPCA_ERR_STATE:
            raise SystemExit(STRAT_NEEDS_RESIDENT) from None
        raise
    n_lab = int((labels >= 0).sum())
    if a.gpca_freq_strat:
        _log(f"genotype counts of {len(rows)} SNPs in {P} groups ({n_lab} of {len(sample_ids)} samples), written to {a.output_prefix}.frq.strat")
    if a.gpca_fst is not None:
        sums = hud[:len(pairs)] if a.gpca_fst == "hudson" else (np.vstack([wcp[:len(pairs)], wcj[None]]) if P > 2 else wcp[:len(pairs)])
        gio.write_fst_summary(a.output_prefix, a.gpca_fst, names, sums)
        _log(f"{a.gpca_fst} Fst of {len(pairs)} pairs of groups over {len(rows)} SNPs, written to {a.output_prefix}.fst.summary")
    if fstat and B >= 1:
        if a.gpca_f2:
            gio.write_f2_summary(a.output_prefix, names, GpcaEngine.fstat(facc, fcnt, [(j, i, j, i) for j, i in pairs]))
            _log(f"f2 of {len(pairs)} pairs of groups over {len(rows)} SNPs in {B} jackknife blocks ({spec}), written to "
                 f"{a.output_prefix}.f2.summary")
        if a.gpca_fstats is not None:
            lst = a.gpca_fstats_list
            gio.write_fstats(a.output_prefix, names, lst, GpcaEngine.fstat(facc, fcnt, [gio.fstat_quad(k, g) for k, g in lst]))
            _log(f"{len(lst)} f-statistics over {len(rows)} SNPs in {B} jackknife blocks ({spec}), written to {a.output_prefix}.fstats")


def _cc_freq(eng, a, fs, rows, Yb, bnames, include):
    """--gpca-assoc-cc-freq: the genotype counts of every SNP among the controls and the cases of every case / control trait, over the
    scan's include set (label -1 outside it), into P.<trait>.frq.cc in the .frq.strat format."""
    for t, name in enumerate(bnames):
        labels = np.where(include, Yb[:, t].astype(np.int32), -1).astype(np.int32)
        for bi, (r0, r1) in enumerate(gio.group_count_bands(len(rows), 2)):
            c = eng.group_counts(labels, 2, rows=(r0, r1))
            gio.write_frq_strat(f"{a.output_prefix}.{name}.frq.cc", *_snp_meta(fs, rows[r0:r1]), ["CTRL", "CASE"], c, append=bi > 0)
    _log(f"case / control genotype counts of {len(rows)} SNPs for {len(bnames)} traits, written to {a.output_prefix}.<trait>.frq.cc")


ASSOC_NEEDS_RESIDENT = ("error: --gpca-assoc-pheno needs the genotype matrix resident on the device: the scan of a matrix walked out of "
                        "core is not implemented")
ASSOC_MAX_COLUMNS = 64
# why gpca_logistic_null refuses a trait, by status (BAD_ARG, NOT_CONVERGED)
LOGISTIC_NULL_FAILURES = {-1: "the included samples hold one class only, or a covariate is constant or collinear over them",
                          -6: "Newton's method does not converge: the covariates separate the cases from the controls"}


def _assoc_tables(a):
    """The phenotype and covariate tables of --gpca-assoc-pheno / --gpca-assoc-covar, read once before any work on the device; refuses
    more than 64 columns (traits + PCs + covariates; with --gpca-assoc-logistic the quantitative traits only, and PCs + covariates + 3
    when a column is binary).  Returns (pheno, covar or None)."""
    def table(flag, path):
        try:
            return gio.read_pheno(path)
        except OSError:
            raise SystemExit(f"error: {flag}: cannot open {path}") from None
        except ValueError as e:
            raise SystemExit(f"error: {flag}: {e}") from None
    pheno = table("--gpca-assoc-pheno", a.gpca_assoc_pheno)
    covar = None if a.gpca_assoc_covar is None else table("--gpca-assoc-covar", a.gpca_assoc_covar)
    t, c = len(pheno.names), 0 if covar is None else len(covar.names)
    p = a.eigensnp_k_global if a.gpca_assoc_pcs is None else a.gpca_assoc_pcs
    if a.gpca_assoc_logistic:
        nb = sum(gio.binary_trait(pheno.values[:, j]) is not None for j in range(t))
        if nb and p + c + 3 > ASSOC_MAX_COLUMNS:
            raise SystemExit(f"error: --gpca-assoc-logistic: {p} PCs + {c} covariates + 3 are more than {ASSOC_MAX_COLUMNS} columns")
        t -= nb                                                                      # the linear scan takes the quantitative traits
    if t + p + c > ASSOC_MAX_COLUMNS:
        raise SystemExit(f"error: --gpca-assoc-pheno: {t} traits + {p} PCs + {c} covariates are more than {ASSOC_MAX_COLUMNS} columns")
    return pheno, covar


def _assoc(eng, a, fs, cols, sample_ids, scores, inset, st, l2=None):
    """--gpca-assoc-pheno FILE: the linear association scan (gpca_assoc_linear) of every SNP that passes the SNP QC, in row bands, into
    P.<trait>.assoc.linear.  Runs last: it resets the keep mask to the QC mask (mu, sigma unchanged), which ends the fit's validity.
    Covariates = the first P columns of the scores the run wrote, then the columns of --gpca-assoc-covar; a sample is included when
    every trait and covariate is present for it and it is in the KING in-set, when there is one."""
    from . import _lib
    pheno, covar = a.gpca_assoc_tables
    fids = fs.family_ids if cols is None else [fs.family_ids[i] for i in cols]
    n = len(sample_ids)
    P = scores.shape[1] if a.gpca_assoc_pcs is None else a.gpca_assoc_pcs
    Y = gio.align_pheno(pheno, fids, sample_ids)
    C = scores[:, :P]
    if covar is not None:
        C = np.hstack([C, gio.align_pheno(covar, fids, sample_ids)])
    C = np.ascontiguousarray(C, np.float64)
    T, Pc = Y.shape[1], C.shape[1]
    include = np.isfinite(Y).all(1) & np.isfinite(C).all(1)
    if inset is not None:
        include &= np.asarray(inset, bool)
    n_inc = int(include.sum())
    df = n_inc - Pc - 2
    if df < 1:
        raise SystemExit(f"error: --gpca-assoc-pheno: {n_inc} samples have every trait and covariate, which leaves no degree of freedom "
                         f"beside {Pc} covariates")
    vif = 50.0 if a.gpca_assoc_vif is None else a.gpca_assoc_vif
    # --gpca-assoc-logistic: the binary columns (recoded to 0 / 1) leave the linear scan for the score scan
    names, bnames, Yb = list(pheno.names), [], np.zeros((n, 0))
    if a.gpca_assoc_logistic:
        coded = [gio.binary_trait(pheno.values[:, j]) for j in range(T)]
        shift = [0.0 if c is None else float(np.nanmin(pheno.values[:, j])) for j, c in enumerate(coded)]
        bcols = [j for j in range(T) if coded[j] is not None]
        bnames = [names[j] for j in bcols]
        Yb = np.ascontiguousarray(np.where(include[:, None], Y[:, bcols] - np.asarray([shift[j] for j in bcols])[None, :], 0.0), np.float64)
        qcols = [j for j in range(T) if coded[j] is None]
        names, Y = [names[j] for j in qcols], np.ascontiguousarray(Y[:, qcols])
        for j, name in enumerate(bnames):                                            # before any file of the trait is written
            try:
                GpcaEngine.logistic_null(Yb[:, j], C, include)
            except _lib.GpcaError as e:
                why = LOGISTIC_NULL_FAILURES.get(e.status, e.message)
                raise SystemExit(f"error: --gpca-assoc-logistic: trait {name}: the null model cannot be fitted ({why})") from None
    T = Y.shape[1]
    eng.set_standardization(st["mu"], st["sigma"], st["keep"])                       # every SNP that passes the SNP QC
    rows = np.flatnonzero(st["keep"])
    lib = _lib.load()
    a1_all = np.full(len(rows), np.nan)                                              # (of every kept row, for the sets' MAF rule)
    spa_z = 2.0 if a.gpca_assoc_spa_z is None else a.gpca_assoc_spa_z
    firth_z = 1.959964 if a.gpca_assoc_firth_z is None else a.gpca_assoc_firth_z
    ldsc = {name: np.full(len(rows), np.nan) for name in pheno.names} if a.gpca_assoc_ldsc else None     # chi2 of every trait

    def meta_of(r0, r1):
        rr = rows[r0:r1]
        return ([fs.chromosomes[i] for i in rr], [int(fs.positions[i]) for i in rr], [fs.variant_ids[i] for i in rr], [fs.allele1[i] for i in rr])
    try:
        if a.gpca_assoc_cc_freq and bnames:
            _cc_freq(eng, a, fs, rows, Yb, bnames, include)
        for bi, (r0, r1) in enumerate(gio.assoc_bands(len(rows), T + Pc) if T else []):
            r = eng.assoc_linear(Y, C, include=include, max_vif=vif, rows=(r0, r1))
            meta = meta_of(r0, r1)
            for t, name in enumerate(names):
                tt = r["t"][:, t]
                lp = [float("nan") if v != v else lib.gpca_student_t_log10p(float(v), float(df)) for v in tt]
                gio.write_assoc(a.output_prefix, name, *meta, r["n_obs"], r["a1_freq"], r["beta"][:, t], r["se"][:, t], tt, lp, append=bi > 0)
                if ldsc is not None:
                    ldsc[name][r0:r1] = tt * tt
        for t0, t1 in (gio.assoc_score_groups(len(bnames), Pc) if bnames else []):
            Yg = np.ascontiguousarray(Yb[:, t0:t1])
            for bi, (r0, r1) in enumerate(gio.assoc_score_bands(len(rows), t1 - t0, Pc)):
                if a.gpca_assoc_firth:
                    r = eng.assoc_logistic_firth(Yg, C, include=include, max_vif=vif, firth_z=firth_z, rows=(r0, r1))
                elif a.gpca_assoc_spa:
                    r = eng.assoc_logistic_spa(Yg, C, include=include, max_vif=vif, spa_z=spa_z, rows=(r0, r1))
                else:
                    r = eng.assoc_logistic_score(Yg, C, include=include, max_vif=vif, rows=(r0, r1))
                meta = meta_of(r0, r1)
                a1_all[r0:r1] = r["a1_freq"]
                for t in range(t1 - t0):
                    zz, beta, se, spa, firth = r["z"][:, t], r["beta"][:, t], r["se"][:, t], None, None
                    if a.gpca_assoc_firth:
                        lp, firth = r["log10p"][:, t], r["firth_status"][:, t]
                        beta, se = np.where(firth == 1, r["firth_beta"][:, t], beta), np.where(firth == 1, r["firth_se"][:, t], se)
                    elif a.gpca_assoc_spa:
                        lp, spa = r["log10p"][:, t], r["spa_status"][:, t]
                    else:
                        lp = [float("nan") if v != v else lib.gpca_normal_log10p(float(v)) for v in zz]
                    gio.write_assoc_logistic(a.output_prefix, bnames[t0 + t], *meta, r["n_obs"], r["a1_freq"], beta, se, zz,
                                             lp, append=bi > 0, spa=spa, firth=firth)
                    if ldsc is not None:
                        ldsc[bnames[t0 + t]][r0:r1] = zz * zz
        if a.gpca_assoc_set_list is not None and bnames:
            _assoc_sets(eng, a, fs, rows, a1_all, Yb, bnames, C, Pc, include, vif)
    except _lib.GpcaError as e:
        if e.status == _lib.GPCA_ERR_STATE:
            raise SystemExit(ASSOC_NEEDS_RESIDENT) from None
        raise
    _log(f"association scan of {len(rows)} SNPs against {T} traits with {Pc} covariates ({P} PCs) on {n_inc} of {n} samples, written to "
         f"{a.output_prefix}.<trait>.assoc.linear")
    if bnames:
        _log(f"logistic score scan of {len(rows)} SNPs against {len(bnames)} case / control traits with {Pc} covariates on {n_inc} of {n} "
             f"samples, written to {a.output_prefix}.<trait>.assoc.logistic")
    if ldsc is not None:
        # --gpca-assoc-ldsc: one LD-score regression per trait in file order; chi2 = T_STAT^2 or the score Z_STAT^2, NaN rows drop out
        out = []
        for name in pheno.names:
            try:
                fit = GpcaEngine.ldsc_fit(ldsc[name], l2, n_inc, len(rows), n_blocks=200, chi2_max=max(0.001 * n_inc, 80.0))
            except _lib.GpcaError:
                fit = None
                print(f"note: --gpca-assoc-ldsc: trait {name}: too few SNPs with a statistic, or LD scores without spread: NA", file=sys.stderr)
            out.append((name, "LOGISTIC" if name in bnames else "LINEAR", n_inc, fit))
        gio.write_ldsc_summary(a.output_prefix, out)
        _log(f"LD-score regression of {len(out)} traits over {len(rows)} SNPs, written to {a.output_prefix}.ldsc.summary")


QTL_NEEDS_RESIDENT = ("error: --gpca-qtl-pheno needs the genotype matrix resident on the device: the scan of a matrix walked out of "
                      "core is not implemented")
QTL_MAX_COVARIATES = 63
QTL_MAX_TRAITS = 1 << 20
QTL_CAP = 1 << 20


def _qtl_tables(a):
    """The trait and covariate tables of --gpca-qtl-pheno / --gpca-qtl-covar, read once before any work on the device; refuses more than
    2^20 traits and more than 63 covariates (PCs + columns).  Returns (pheno, covar or None)."""
    def table(flag, path):
        try:
            return gio.read_pheno(path)
        except OSError:
            raise SystemExit(f"error: {flag}: cannot open {path}") from None
        except ValueError as e:
            raise SystemExit(f"error: {flag}: {e}") from None
    pheno = table("--gpca-qtl-pheno", a.gpca_qtl_pheno)
    covar = None if a.gpca_qtl_covar is None else table("--gpca-qtl-covar", a.gpca_qtl_covar)
    t, c = len(pheno.names), 0 if covar is None else len(covar.names)
    p = a.eigensnp_k_global if a.gpca_qtl_pcs is None else a.gpca_qtl_pcs
    if t > QTL_MAX_TRAITS:
        raise SystemExit(f"error: --gpca-qtl-pheno: {t} traits are more than {QTL_MAX_TRAITS}")
    if p + c > QTL_MAX_COVARIATES:
        raise SystemExit(f"error: --gpca-qtl-pheno: {p} PCs + {c} covariates are more than {QTL_MAX_COVARIATES} covariates")
    return pheno, covar


def _qtl(eng, a, fs, cols, sample_ids, scores, inset, st):
    """--gpca-qtl-pheno FILE: the many-trait QTL scan (gpca_assoc_qtl) of every SNP that passes the SNP QC against every column of FILE,
    in row bands, into P.qtl.hits (the pairs at or beyond the threshold, in (SNP, trait) order) and P.qtl.best (the best SNP of every
    trait).  Runs last, after the association scan: it resets the keep mask to the QC mask.  Covariates and the include rule are the
    association scan's.  The threshold on -log10 p becomes one on |t| once (gpca_qtl_t_min) and that one on r2.  The statistics of a hit
    come from gpca_qtl_stats; those of a trait's best SNP from gpca_assoc_linear on that SNP, which gives the same bits."""
    from . import _lib
    pheno, covar = a.gpca_qtl_tables
    fids = fs.family_ids if cols is None else [fs.family_ids[i] for i in cols]
    n = len(sample_ids)
    P = scores.shape[1] if a.gpca_qtl_pcs is None else a.gpca_qtl_pcs
    Y = np.ascontiguousarray(gio.align_pheno(pheno, fids, sample_ids), np.float64)
    C = scores[:, :P]
    if covar is not None:
        C = np.hstack([C, gio.align_pheno(covar, fids, sample_ids)])
    C = np.ascontiguousarray(C, np.float64)
    T, Pc = Y.shape[1], C.shape[1]
    include = np.isfinite(Y).all(1) & np.isfinite(C).all(1)
    if inset is not None:
        include &= np.asarray(inset, bool)
    n_inc = int(include.sum())
    df = n_inc - Pc - 2
    if df < 1:
        raise SystemExit(f"error: --gpca-qtl-pheno: {n_inc} samples have every trait and covariate, which leaves no degree of freedom "
                         f"beside {Pc} covariates")
    vif = 50.0 if a.gpca_qtl_vif is None else a.gpca_qtl_vif
    lib = _lib.load()
    tmin = a.gpca_qtl_t if a.gpca_qtl_t is not None else float(lib.gpca_qtl_t_min(5.0 if a.gpca_qtl_log10p is None else a.gpca_qtl_log10p, float(df)))
    if not tmin < float("inf"):
        raise SystemExit(f"error: --gpca-qtl-log10p: no finite t reaches the threshold at {df} degrees of freedom")
    r2_min = tmin * tmin / (tmin * tmin + df)
    eng.set_standardization(st["mu"], st["sigma"], st["keep"])                       # every SNP that passes the SNP QC
    rows = np.flatnonzero(st["keep"])
    names = list(pheno.names)
    if not a.gpca_qtl_cis_only:
        _qtl_trans(eng, a, fs, lib, Y, C, include, vif, r2_min, tmin, rows, names, T, Pc, P, n, n_inc, df)
    if a.gpca_qtl_cis_pos is not None:
        _qtl_cis(eng, a, fs, Y, C, include, vif, rows, names, T, Pc, n, n_inc, df)


def _qtl_trans(eng, a, fs, lib, Y, C, include, vif, r2_min, tmin, rows, names, T, Pc, P, n, n_inc, df):
    """The scan of every SNP against every trait of _qtl, into P.qtl.hits and P.qtl.best."""
    from . import _lib
    b2, bw = np.full(T, np.nan), np.full(T, -1, np.int64)
    n_tests, n_hits = 0, 0
    log10p = lambda t: float("nan") if t != t else lib.gpca_student_t_log10p(float(t), float(df))
    try:
        for bi, (r0, r1) in enumerate(gio.assoc_qtl_bands(len(rows), T, n, QTL_CAP)):
            q = eng.assoc_qtl(Y, C, include=include, max_vif=vif, r2_min=r2_min, cap=QTL_CAP, rows=(r0, r1))
            if q["n_found"] > QTL_CAP:                                               # a band with more hits than the buffer: once more
                q = eng.assoc_qtl(Y, C, include=include, max_vif=vif, r2_min=r2_min, cap=q["n_found"], rows=(r0, r1))
            with np.errstate(invalid="ignore"):
                n_tests += int((~((q["n_obs"] == 0) | ~(q["xx"] > 0.0) | (q["sxx"] * vif < q["xx"]))).sum())
            hr, ht = q["rows"].astype(np.int64), q["traits"].astype(np.int64)
            stt = GpcaEngine.qtl_stats(q["xb"], q["sxx"][hr - r0], q["yy"][ht], df)
            o = rows[hr]
            gio.write_qtl_hits(a.output_prefix, [fs.chromosomes[i] for i in o], [int(fs.positions[i]) for i in o], [fs.variant_ids[i] for i in o],
                               [fs.allele1[i] for i in o], [names[t] for t in ht], q["n_obs"][hr - r0], q["a1_freq"][hr - r0], stt[:, 0], stt[:, 1],
                               stt[:, 2], [log10p(t) for t in stt[:, 2]], append=bi > 0)
            n_hits += q["n_found"]
            gio.qtl_best_merge(b2, bw, q["best_r2"], q["best_row"])
        if len(rows) == 0:
            gio.write_qtl_hits(a.output_prefix, [], [], [], [], [], [], [], [], [], [], [])
        # the best SNP of every trait: gpca_assoc_linear on that SNP, the traits that share a SNP in groups of 64 - Pc
        beta, se, tt = np.full(T, np.nan), np.full(T, np.nan), np.full(T, np.nan)
        for r in np.unique(bw[bw >= 0]):
            ts = np.flatnonzero(bw == r)
            for g0 in range(0, len(ts), 64 - Pc):
                g = ts[g0:g0 + 64 - Pc]
                res = eng.assoc_linear(np.ascontiguousarray(Y[:, g]), C, include=include, max_vif=vif, rows=(int(r), int(r) + 1))
                beta[g], se[g], tt[g] = res["beta"][0], res["se"][0], res["t"][0]
    except _lib.GpcaError as e:
        if e.status == _lib.GPCA_ERR_STATE:
            raise SystemExit(QTL_NEEDS_RESIDENT) from None
        raise
    ob = [None if r < 0 else int(rows[r]) for r in bw]
    pick = lambda col: [None if i is None else col[i] for i in ob]
    gio.write_qtl_best(a.output_prefix, names, pick(fs.chromosomes), [0 if i is None else int(fs.positions[i]) for i in ob], pick(fs.variant_ids),
                       pick(fs.allele1), beta, se, tt, [log10p(t) for t in tt], [n_tests if i is not None else 0 for i in ob])
    _log(f"QTL scan of {len(rows)} SNPs against {T} traits with {Pc} covariates ({P} PCs) on {n_inc} of {n} samples: {n_hits} pairs with "
         f"|t| >= {tmin:.6g}, written to {a.output_prefix}.qtl.hits and {a.output_prefix}.qtl.best")


def _qtl_cis(eng, a, fs, Y, C, include, vif, rows, names, T, Pc, n, n_inc, df):
    """--gpca-qtl-cis-pos FILE: cis-QTL mapping (gpca_assoc_qtl_cis) of every trait of --gpca-qtl-pheno that FILE gives a position,
    against the SNPs that pass the SNP QC within --gpca-qtl-cis-window of it, with --gpca-qtl-cis-perm permutations from the table of
    --gpca-qtl-cis-seed, in bands of traits, into P.qtl.cis.  Samples, covariates and refusals are the scan's."""
    from . import _lib
    window = 1000000 if a.gpca_qtl_cis_window is None else a.gpca_qtl_cis_window
    nperm = 1000 if a.gpca_qtl_cis_perm is None else a.gpca_qtl_cis_perm
    seed = 0 if a.gpca_qtl_cis_seed is None else a.gpca_qtl_cis_seed
    tpos = [a.gpca_qtl_cis_table.get(t) for t in names]
    chrom = [fs.chromosomes[i] for i in rows]
    pos = [int(fs.positions[i]) for i in rows]
    try:
        win = gio.qtl_cis_windows(chrom, pos, ["" if p is None else p[0] for p in tpos], [0 if p is None else p[1] for p in tpos], window)
    except ValueError as e:
        raise SystemExit(f"error: --gpca-qtl-cis-pos: {e}") from None
    for g, p in enumerate(tpos):
        if p is None:
            win[g] = 0
    perm = GpcaEngine.qtl_perm_table(seed, n_inc, nperm)
    parts = []
    try:
        # (no SNP passes the SNP QC: nothing to ask the device; every trait with a position gets its N_VAR = 0 line)
        for g0, g1 in (gio.assoc_qtl_cis_bands(T, nperm) if len(rows) else []):
            parts.append(eng.assoc_qtl_cis(np.ascontiguousarray(Y[:, g0:g1]), win[g0:g1], C, include=include, max_vif=vif, perm=perm))
    except _lib.GpcaError as e:
        if e.status == _lib.GPCA_ERR_STATE:
            raise SystemExit(QTL_NEEDS_RESIDENT) from None
        raise
    res = {k: np.concatenate([q[k] for q in parts]) for k in ("n_var", "best_row", "best_r2", "best_stat", "perm_r2")} if parts else \
        {"n_var": np.zeros(T, np.int64), "best_row": np.full(T, -1, np.int64), "best_r2": np.full(T, np.nan), "best_stat": np.full((T, 3), np.nan),
         "perm_r2": np.full((T, nperm), np.nan)}
    res["df"] = float(df)
    gio.write_qtl_cis(a.output_prefix, names, tpos, res, [fs.variant_ids[i] for i in rows], pos, [fs.allele1[i] for i in rows])
    n_pos = sum(p is not None for p in tpos)
    _log(f"cis-QTL mapping of {n_pos} of {T} traits within {window} bp with {Pc} covariates on {n_inc} of {n} samples and {nperm} "
         f"permutations (seed {seed}), written to {a.output_prefix}.qtl.cis")


def _assoc_sets(eng, a, fs, rows, a1_freq, Yb, bnames, C, Pc, include, vif):
    """--gpca-assoc-set-list FILE: the gene-level burden and SKAT tests (gpca_assoc_logistic_set, gpca_set_test) of every case / control
    trait, on the QC mask and the include set of the per-SNP scans, into P.<trait>.assoc.set; one row per set in file order."""
    sets = gio.read_set_list(a.gpca_assoc_set_list, [fs.variant_ids[i] for i in rows])
    max_maf = 0.01 if a.gpca_assoc_set_max_maf is None else a.gpca_assoc_set_max_maf
    kind = "beta" if a.gpca_assoc_set_weights is None else a.gpca_assoc_set_weights
    enter = gio.set_maf_ok(a1_freq, max_maf)
    left = [s.rows[enter[s.rows]] for s in sets]
    n_var = [len(r) for r in left]
    for s, m in zip(sets, n_var):
        if m > gio.ASSOC_SET_MAX_ROWS:
            print(f"note: --gpca-assoc-set-list: set {s.name} keeps {m} variants, more than {gio.ASSOC_SET_MAX_ROWS}: NA", file=sys.stderr)
    run = [i for i, m in enumerate(n_var) if 1 <= m <= gio.ASSOC_SET_MAX_ROWS]
    results = [[None] * len(sets) for _ in bnames]
    for t0, t1 in gio.assoc_score_groups(len(bnames), Pc):
        Yg = np.ascontiguousarray(Yb[:, t0:t1])
        for s0, s1 in gio.assoc_set_groups([n_var[i] for i in run], t1 - t0, Pc):
            r = eng.assoc_logistic_set(Yg, [left[i] for i in run[s0:s1]], C, include=include, max_vif=vif, ua=True)
            for k, i in enumerate(run[s0:s1]):
                lo, hi = int(r["set_off"][k]), int(r["set_off"][k + 1])
                sg = np.where(r["flipped"][lo:hi] == 1, -1.0, 1.0)
                w = gio.set_weights(r["a1_freq"][lo:hi], kind)
                for t in range(t1 - t0):
                    results[t0 + t][i] = GpcaEngine.set_test(sg * r["ua"][lo:hi, t, 0], r["phi"][k][t], w)
    for t, name in enumerate(bnames):
        gio.write_assoc_set(a.output_prefix, name, [s.name for s in sets], [s.chrom for s in sets], [s.pos for s in sets], n_var, results[t])
    _log(f"set tests of {len(run)} of {len(sets)} sets against {len(bnames)} case / control traits, written to "
         f"{a.output_prefix}.<trait>.assoc.set")


def _indep_pairwise(eng, a, fs, st, keep, by_tag):
    """--gpca-indep-pairwise WINDOW R2: the threshold bits of the windowed r^2 (gpca_ld_window, in row bands), the pruning rule
    (io.ld_prune) and P.prune.in / P.prune.out; the in-set narrows the keep mask (mu, sigma unchanged) and the block lists.  Returns
    the new (keep, by_tag)."""
    from . import _lib
    window, r2max = a.gpca_indep_pairwise[0], float(a.gpca_indep_pairwise[1])
    rows = np.flatnonzero(keep)
    try:
        win_end = gio.ld_windows([fs.chromosomes[r] for r in rows], np.asarray(fs.positions, np.int64)[rows], window)
    except ValueError as e:
        raise SystemExit(f"error: --gpca-indep-pairwise: {e} (variant indices count the SNPs kept by QC and the LD blocks)") from None
    counts, _ = eng.snp_qc_detail()
    counts = counts[rows]
    maf = gio.maf_from_qc_detail(counts[:, 0], counts[:, 2], counts[:, 3])

    def bands():
        for r0, r1, wm in gio.ld_bands(win_end):
            yield (r0, r1), eng.ld_window(win_end[r0:r1], wmax=wm, rows=(r0, r1), threshold=r2max, r2=False)["above"]
    try:
        inset = gio.ld_prune(win_end, bands(), maf)
    except _lib.GpcaError as e:
        if e.status == _lib.GPCA_ERR_STATE:
            raise SystemExit("error: --gpca-indep-pairwise needs the genotype matrix resident on the device: with the matrix walked out "
                             "of core a window crosses the panels, and the halo of rows that needs is not implemented") from None
        raise
    _ensure_parent(a.output_prefix)
    gio.write_prune_ids(a.output_prefix, [fs.variant_ids[r] for r in rows], inset)
    _log(f"LD pruning (window {window}, r^2 > {r2max:g}): {int(inset.sum())} SNPs kept, {len(rows) - int(inset.sum())} removed")
    keep2 = np.zeros_like(keep)
    keep2[rows[inset]] = 1
    eng.set_standardization(st["mu"], st["sigma"], keep2)
    by_tag = [(t, [r for r in rs if keep2[r]]) for t, rs in by_tag]
    return keep2, [(t, rs) for t, rs in by_tag if rs]


def run_project_workflow(a) -> int:
    """--gpca-project-model MODEL --bed-file TARGET --out Q: the target's samples on the model's PCs (gpca_project)."""
    if not a.bed_file:
        raise SystemExit("error: --bed-file is required with --gpca-project-model")
    if a.eigensnp or a.vcf_dir:
        raise SystemExit("error: --gpca-project-model takes a --bed-file target, not --eigensnp or --vcf-dir")
    if a.gpca_precision != "i8":
        raise SystemExit("error: --gpca-project-model needs --gpca-precision i8")
    t0 = time.time()
    model = gio.read_model(a.gpca_project_model)
    fs = gio.read_plink(a.bed_file)
    al = gio.align_model(model, fs.variant_ids, fs.allele1, fs.allele2)
    _log(f"model of {len(model.variant_ids)} SNPs, k = {model.k}: {al.matched} matched ({al.flipped} with swapped alleles), "
         f"{al.allele_mismatch} allele mismatches dropped, {al.absent} absent from the target")
    if al.matched == 0:
        raise SystemExit(f"error: no SNP of {a.gpca_project_model} matches a variant of {a.bed_file} (by ID and alleles)")
    prec, store = _engine_modes(a, fs.n_samples)
    with GpcaEngine(device=a.device, precision=prec, storage=store) as eng:
        _load_bed(eng, a, fs, None)
        scores, used = eng.project(al.mean, al.sd, al.loadings)
    _ensure_parent(a.output_prefix)
    gio.write_projected(a.output_prefix, fs.sample_ids, scores, used)
    _log(f"projection of {fs.n_samples} samples done in {time.time() - t0:.2f}s")
    return 0


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    if a.gpca_make_grm and not a.eigensnp:
        raise SystemExit("error: --gpca-make-grm needs the --eigensnp workflow")
    if (a.gpca_make_king or a.gpca_king_cutoff is not None) and not a.eigensnp:
        raise SystemExit("error: --gpca-make-king and --gpca-king-cutoff need the --eigensnp workflow")
    if a.gpca_king_table_filter is not None and not a.gpca_make_king:
        raise SystemExit("error: --gpca-king-table-filter needs --gpca-make-king")
    if a.gpca_king_cutoff is not None and not 0.0 < a.gpca_king_cutoff < 0.5:
        raise SystemExit("error: --gpca-king-cutoff must lie in (0, 0.5)")
    if a.gpca_king_cutoff is not None and a.gpca_eigensnp_local_stage:
        raise SystemExit("error: --gpca-king-cutoff cannot be combined with --gpca-eigensnp-local-stage (that stage owns the sample mask)")
    if a.gpca_make_pcrelate is None and (a.gpca_pcrelate_maf_bound is not None or a.gpca_pcrelate_table_filter is not None):
        raise SystemExit("error: --gpca-pcrelate-maf-bound and --gpca-pcrelate-table-filter need --gpca-make-pcrelate")
    if a.gpca_make_pcrelate is not None:
        if not a.eigensnp:
            raise SystemExit("error: --gpca-make-pcrelate needs the --eigensnp workflow")
        if not 0 <= a.gpca_make_pcrelate <= min(a.eigensnp_k_global, 32):
            raise SystemExit("error: --gpca-make-pcrelate P must lie in [0, min(--eigensnp-k-global, 32)]")
        if a.gpca_pcrelate_maf_bound is not None and not 0.0 <= a.gpca_pcrelate_maf_bound < 0.5:
            raise SystemExit("error: --gpca-pcrelate-maf-bound must lie in [0, 0.5)")
        if a.gpca_eigensnp_local_stage:
            raise SystemExit("error: --gpca-make-pcrelate cannot be combined with --gpca-eigensnp-local-stage (that stage defines no "
                             "all-sample scores)")
        if a.gpca_stream == "on":
            raise SystemExit(PCRELATE_NEEDS_RESIDENT)
    if a.gpca_assoc_pheno is None and (a.gpca_assoc_pcs is not None or a.gpca_assoc_covar is not None or a.gpca_assoc_vif is not None):
        raise SystemExit("error: --gpca-assoc-pcs, --gpca-assoc-covar and --gpca-assoc-vif need --gpca-assoc-pheno")
    if a.gpca_assoc_logistic and a.gpca_assoc_pheno is None:
        raise SystemExit("error: --gpca-assoc-logistic needs --gpca-assoc-pheno")
    if a.gpca_assoc_spa and not a.gpca_assoc_logistic:
        raise SystemExit("error: --gpca-assoc-spa needs --gpca-assoc-logistic")
    if a.gpca_assoc_spa_z is not None and not a.gpca_assoc_spa:
        raise SystemExit("error: --gpca-assoc-spa-z needs --gpca-assoc-spa")
    if a.gpca_assoc_spa_z is not None and not gio.spa_z_ok(a.gpca_assoc_spa_z):
        raise SystemExit("error: --gpca-assoc-spa-z must be at least 0.5, or inf for no correction")
    if a.gpca_assoc_firth and not a.gpca_assoc_logistic:
        raise SystemExit("error: --gpca-assoc-firth needs --gpca-assoc-logistic")
    if a.gpca_assoc_firth and a.gpca_assoc_spa:
        raise SystemExit("error: --gpca-assoc-firth and --gpca-assoc-spa exclude each other")
    if a.gpca_assoc_firth_z is not None and not a.gpca_assoc_firth:
        raise SystemExit("error: --gpca-assoc-firth-z needs --gpca-assoc-firth")
    if a.gpca_assoc_firth_z is not None and not gio.firth_z_ok(a.gpca_assoc_firth_z):
        raise SystemExit("error: --gpca-assoc-firth-z must be at least 0, or inf for no correction")
    if a.gpca_assoc_set_list is not None and not a.gpca_assoc_logistic:
        raise SystemExit("error: --gpca-assoc-set-list needs --gpca-assoc-logistic")
    if a.gpca_assoc_set_list is None and (a.gpca_assoc_set_max_maf is not None or a.gpca_assoc_set_weights is not None):
        raise SystemExit("error: --gpca-assoc-set-max-maf and --gpca-assoc-set-weights need --gpca-assoc-set-list")
    if a.gpca_assoc_set_max_maf is not None and not (0.0 < a.gpca_assoc_set_max_maf <= 0.5):
        raise SystemExit("error: --gpca-assoc-set-max-maf must lie in (0, 0.5]")
    if a.gpca_assoc_set_weights is not None and a.gpca_assoc_set_weights not in ("beta", "flat"):
        raise SystemExit("error: --gpca-assoc-set-weights must be beta or flat")
    if a.gpca_assoc_cc_freq and not a.gpca_assoc_logistic:
        raise SystemExit("error: --gpca-assoc-cc-freq needs --gpca-assoc-logistic")
    if a.gpca_within is None and (a.gpca_freq_strat or a.gpca_fst is not None):
        raise SystemExit("error: --gpca-freq-strat and --gpca-fst need --gpca-within")
    if a.gpca_within is None and (_fstat_asked(a) or a.gpca_fstat_block is not None):
        raise SystemExit("error: --gpca-f2, --gpca-fstats and --gpca-fstat-block need --gpca-within")
    if a.gpca_fstat_block is not None and not _fstat_asked(a):
        raise SystemExit("error: --gpca-fstat-block needs --gpca-f2 or --gpca-fstats")
    if _fstat_asked(a):
        try:
            gio.parse_ld_window(a.gpca_fstat_block if a.gpca_fstat_block is not None else gio.FSTAT_BLOCK_DEFAULT)
        except ValueError:
            raise SystemExit(f"error: --gpca-fstat-block: '{a.gpca_fstat_block}' is neither a variant count such as 500 nor a span such as "
                             "5000kb") from None
    if a.gpca_fst_variants and a.gpca_fst is None:
        raise SystemExit("error: --gpca-fst-variants needs --gpca-fst")
    if a.gpca_fst is not None and a.gpca_fst not in ("hudson", "wc"):
        raise SystemExit("error: --gpca-fst must be hudson or wc")
    if a.gpca_within is not None:
        if not a.eigensnp:
            raise SystemExit("error: --gpca-within needs the --eigensnp workflow")
        if not _strat_asked(a) and not a.gpca_admixture_supervised:
            raise SystemExit("error: --gpca-within needs --gpca-freq-strat or --gpca-fst")
        if a.gpca_stream == "on" and _strat_asked(a):
            raise SystemExit(STRAT_NEEDS_RESIDENT)
        a.gpca_within_table = _within_table(a)
    if _sample_qc_asked(a):
        if not a.eigensnp:
            raise SystemExit("error: --gpca-sample-missing, --gpca-het, --gpca-mind and --gpca-het-sd need the --eigensnp workflow")
        if a.gpca_mind is not None and not 0.0 <= a.gpca_mind < 1.0:
            raise SystemExit("error: --gpca-mind must lie in [0, 1)")
        if a.gpca_het_sd is not None and not (0.0 < a.gpca_het_sd < float("inf")):
            raise SystemExit("error: --gpca-het-sd must be finite and above 0")
        if (a.gpca_mind is not None or a.gpca_het_sd is not None) and a.gpca_eigensnp_local_stage:
            raise SystemExit("error: --gpca-mind and --gpca-het-sd cannot be combined with --gpca-eigensnp-local-stage (that stage owns "
                             "the sample mask)")
        if a.gpca_stream == "on":
            raise SystemExit(SAMPLE_QC_NEEDS_RESIDENT)
    if a.gpca_admixture is None and (a.gpca_admixture_seed is not None or a.gpca_admixture_max_iter is not None or
                                     a.gpca_admixture_tol is not None or a.gpca_admixture_no_accel or a.gpca_admixture_supervised):
        raise SystemExit("error: --gpca-admixture-seed, -max-iter, -tol, -no-accel and --gpca-admixture-supervised need --gpca-admixture")
    if a.gpca_admixture is not None:
        if not a.eigensnp:
            raise SystemExit("error: --gpca-admixture needs the --eigensnp workflow")
        if not 1 <= a.gpca_admixture <= 16:
            raise SystemExit("error: --gpca-admixture K must lie in [1, 16]")
        if a.gpca_admixture_seed is not None and not 0 <= a.gpca_admixture_seed < 1 << 63:
            raise SystemExit("error: --gpca-admixture-seed must lie in [0, 2^63)")
        if a.gpca_admixture_max_iter is not None and not 0 <= a.gpca_admixture_max_iter < 1 << 31:
            raise SystemExit("error: --gpca-admixture-max-iter must lie in [0, 2^31)")
        if a.gpca_admixture_tol is not None and not (0.0 <= a.gpca_admixture_tol < float("inf")):
            raise SystemExit("error: --gpca-admixture-tol must be finite and at least 0")
        if a.gpca_admixture_supervised:
            if a.gpca_within is None:
                raise SystemExit("error: --gpca-admixture-supervised needs --gpca-within")
            if len(a.gpca_within_table.names) != a.gpca_admixture:
                raise SystemExit(f"error: --gpca-admixture-supervised: K = {a.gpca_admixture} but --gpca-within names "
                                 f"{len(a.gpca_within_table.names)} groups")
        if a.gpca_eigensnp_local_stage:
            raise SystemExit("error: --gpca-admixture cannot be combined with --gpca-eigensnp-local-stage (that stage owns the sample "
                             "mask and the keep mask)")
        if a.gpca_stream == "on":
            raise SystemExit(ADMIX_NEEDS_RESIDENT)
    a.gpca_admixture_cv_ks = None
    if a.gpca_admixture_cv is not None or a.gpca_admixture_cv_seed is not None or a.gpca_admixture_cv_k is not None:
        if a.gpca_admixture is None:
            raise SystemExit("error: --gpca-admixture-cv, --gpca-admixture-cv-seed and --gpca-admixture-cv-k need --gpca-admixture")
        if a.gpca_admixture_cv is None:
            raise SystemExit("error: --gpca-admixture-cv-seed and --gpca-admixture-cv-k need --gpca-admixture-cv")
        if not 2 <= a.gpca_admixture_cv <= 64:
            raise SystemExit("error: --gpca-admixture-cv V must lie in [2, 64]")
        if a.gpca_admixture_cv_seed is not None and not 0 <= a.gpca_admixture_cv_seed < 1 << 63:
            raise SystemExit("error: --gpca-admixture-cv-seed must lie in [0, 2^63)")
        a.gpca_admixture_cv_ks = [a.gpca_admixture]
        if a.gpca_admixture_cv_k is not None:
            if a.gpca_admixture_supervised:
                raise SystemExit("error: --gpca-admixture-cv-k cannot be combined with --gpca-admixture-supervised (the groups fix K)")
            lo, sep, hi = a.gpca_admixture_cv_k.partition("-")
            ok = sep == "-" and lo.isascii() and hi.isascii() and lo.isdigit() and hi.isdigit() and len(lo) <= 2 and len(hi) <= 2
            if not ok or not 1 <= int(lo) <= int(hi) <= 16:
                raise SystemExit("error: --gpca-admixture-cv-k must be A-B with 1 <= A <= B <= 16")
            a.gpca_admixture_cv_ks = sorted(set(range(int(lo), int(hi) + 1)) | {a.gpca_admixture})
    if _homozyg_asked(a):
        if not a.eigensnp:
            raise SystemExit("error: --gpca-homozyg needs the --eigensnp workflow")
        a.gpca_homozyg_params = _homozyg_params(a)
        if a.gpca_stream == "on":
            raise SystemExit(HOMOZYG_NEEDS_RESIDENT)
    if a.gpca_assoc_pheno is not None:
        if not a.eigensnp:
            raise SystemExit("error: --gpca-assoc-pheno needs the --eigensnp workflow")
        if a.gpca_assoc_pcs is not None and not 0 <= a.gpca_assoc_pcs <= a.eigensnp_k_global:
            raise SystemExit("error: --gpca-assoc-pcs P must lie in [0, --eigensnp-k-global]")
        if a.gpca_assoc_vif is not None and not (1.0 <= a.gpca_assoc_vif < float("inf")):
            raise SystemExit("error: --gpca-assoc-vif must be finite and at least 1")
        if a.gpca_eigensnp_local_stage:
            raise SystemExit("error: --gpca-assoc-pheno cannot be combined with --gpca-eigensnp-local-stage (that stage defines no "
                             "all-sample scores)")
        if a.gpca_stream == "on":
            raise SystemExit(ASSOC_NEEDS_RESIDENT)
        a.gpca_assoc_tables = _assoc_tables(a)
        if a.gpca_assoc_set_list is not None:                                        # (its format, before any work on the device)
            try:
                gio.read_set_list(a.gpca_assoc_set_list, [])
            except OSError:
                raise SystemExit(f"error: --gpca-assoc-set-list: cannot open {a.gpca_assoc_set_list}") from None
            except ValueError as e:
                raise SystemExit(f"error: --gpca-assoc-set-list: {e}") from None
    if a.gpca_qtl_pheno is None and any(v is not None for v in (a.gpca_qtl_pcs, a.gpca_qtl_covar, a.gpca_qtl_log10p, a.gpca_qtl_t, a.gpca_qtl_vif)):
        raise SystemExit("error: --gpca-qtl-pcs, --gpca-qtl-covar, --gpca-qtl-log10p, --gpca-qtl-t and --gpca-qtl-vif need --gpca-qtl-pheno")
    if a.gpca_qtl_pheno is not None:
        if not a.eigensnp:
            raise SystemExit("error: --gpca-qtl-pheno needs the --eigensnp workflow")
        if a.gpca_qtl_pcs is not None and not 0 <= a.gpca_qtl_pcs <= a.eigensnp_k_global:
            raise SystemExit("error: --gpca-qtl-pcs P must lie in [0, --eigensnp-k-global]")
        if a.gpca_qtl_vif is not None and not (1.0 <= a.gpca_qtl_vif < float("inf")):
            raise SystemExit("error: --gpca-qtl-vif must be finite and at least 1")
        if a.gpca_qtl_log10p is not None and a.gpca_qtl_t is not None:
            raise SystemExit("error: --gpca-qtl-log10p and --gpca-qtl-t set the same threshold: give one")
        if a.gpca_qtl_log10p is not None and not (0.0 <= a.gpca_qtl_log10p < float("inf")):
            raise SystemExit("error: --gpca-qtl-log10p must be finite and at least 0")
        if a.gpca_qtl_t is not None and not (0.0 <= a.gpca_qtl_t < float("inf")):
            raise SystemExit("error: --gpca-qtl-t must be finite and at least 0")
        if a.gpca_eigensnp_local_stage:
            raise SystemExit("error: --gpca-qtl-pheno cannot be combined with --gpca-eigensnp-local-stage (that stage defines no "
                             "all-sample scores)")
        if a.gpca_stream == "on":
            raise SystemExit(QTL_NEEDS_RESIDENT)
        a.gpca_qtl_tables = _qtl_tables(a)
    if a.gpca_qtl_cis_pos is None and (a.gpca_qtl_cis_only or any(v is not None for v in (a.gpca_qtl_cis_window, a.gpca_qtl_cis_perm, a.gpca_qtl_cis_seed))):
        raise SystemExit("error: --gpca-qtl-cis-window, --gpca-qtl-cis-perm, --gpca-qtl-cis-seed and --gpca-qtl-cis-only need --gpca-qtl-cis-pos")
    if a.gpca_qtl_cis_pos is not None:
        if a.gpca_qtl_pheno is None:
            raise SystemExit("error: --gpca-qtl-cis-pos needs --gpca-qtl-pheno")
        if a.gpca_qtl_cis_window is not None and a.gpca_qtl_cis_window < 0:
            raise SystemExit("error: --gpca-qtl-cis-window must be at least 0")
        if a.gpca_qtl_cis_perm is not None and not 0 <= a.gpca_qtl_cis_perm <= 65535:
            raise SystemExit("error: --gpca-qtl-cis-perm must lie in [0, 65535]")
        if a.gpca_qtl_cis_seed is not None and a.gpca_qtl_cis_seed < 0:
            raise SystemExit("error: --gpca-qtl-cis-seed must be at least 0")
        try:
            a.gpca_qtl_cis_table = gio.read_trait_pos(a.gpca_qtl_cis_pos)
        except OSError:
            raise SystemExit(f"error: --gpca-qtl-cis-pos: cannot open {a.gpca_qtl_cis_pos}") from None
        except ValueError as e:
            raise SystemExit(f"error: --gpca-qtl-cis-pos: {e}") from None
    if a.gpca_indep_pairwise:
        if not a.eigensnp:
            raise SystemExit("error: --gpca-indep-pairwise needs the --eigensnp workflow")
        try:
            gio.parse_ld_window(a.gpca_indep_pairwise[0])
        except ValueError as e:
            raise SystemExit(f"error: --gpca-indep-pairwise: {e}") from None
        try:
            r2max = float(a.gpca_indep_pairwise[1])
        except ValueError:
            r2max = float("nan")
        if not 0.0 < r2max < 1.0:
            raise SystemExit("error: --gpca-indep-pairwise R2 must lie in (0, 1)")
    if a.gpca_assoc_ldsc and (a.gpca_ld_score is None or a.gpca_assoc_pheno is None):
        raise SystemExit("error: --gpca-assoc-ldsc needs --gpca-ld-score and --gpca-assoc-pheno")
    if a.gpca_ld_score is not None:
        if not a.eigensnp:
            raise SystemExit("error: --gpca-ld-score needs the --eigensnp workflow")
        try:
            gio.parse_ld_window(a.gpca_ld_score)
        except ValueError as e:
            raise SystemExit(f"error: --gpca-ld-score: {e}") from None
        if a.gpca_stream == "on":
            raise SystemExit(LD_SCORE_NEEDS_RESIDENT)
    if a.gpca_project_model:
        return run_project_workflow(a)
    if a.gpca_save_model and not a.eigensnp:
        raise SystemExit("error: --gpca-save-model needs the --eigensnp workflow")
    return run_eigensnp_workflow(a) if a.eigensnp else run_vcf_workflow(a)


if __name__ == "__main__":
    sys.exit(main())
