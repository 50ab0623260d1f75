"""genomic_pca_amd -- MI355X-native randomized PCA for genotype matrices (hot path of SauersML/genomic_pca).

Product code: libgpca.so (HIP, gfx950) behind include/gpca.h + this thin host mirror.  No CPU fallback."""
from ._lib import GpcaError, GpcaLibraryError, LIB_PATH, build, load  # noqa: F401
from .engine import (EigenSNPCoreAlgorithm, EigenSNPCoreAlgorithmConfig, EigenSNPCoreOutput, GpcaEngine,  # noqa: F401
                     LdBlockSpecification, MicroarrayGenotypeAccessor, PCA, PanelSource, QcConfig)
from .synth import synth_thresholds, synth_thresholds16  # noqa: F401
from .distributed import shard_rows  # noqa: F401

spa_log10p = GpcaEngine.spa_log10p
firth_log10p = GpcaEngine.firth_log10p
set_test = GpcaEngine.set_test
fst_hudson = GpcaEngine.fst_hudson
fst_wc = GpcaEngine.fst_wc
het_weights = GpcaEngine.het_weights
sample_het = GpcaEngine.sample_het
roh_select = GpcaEngine.roh_select
roh_threshold = GpcaEngine.roh_threshold
admix_cv_fold = GpcaEngine.admix_cv_fold
qtl_stats = GpcaEngine.qtl_stats
qtl_t_min = GpcaEngine.qtl_t_min
qtl_perm_table = GpcaEngine.qtl_perm_table
qtl_perm_panel = GpcaEngine.qtl_perm_panel      # (engine, b, Q, perm): it runs on the engine's device
qtl_beta_approx = GpcaEngine.qtl_beta_approx

__version__ = "0.2.2"
