/*
 * gpca.h -- C ABI of the MI355X-native randomized-PCA engine (libgpca.so).
 *
 * Drop-in boundary for ONE hot path of SauersML/genomic_pca: per-SNP standardisation fused into
 * the randomized-SVD core.  Plain C types only: opaque handle, caller-owned host buffers,
 * integer status codes, no exceptions, no C++/torch types.  A Rust host binds these with a
 * 30-line `extern "C"` block.
 *
 * The reference's seam is a PULL model (the solver calls the accessor for f32 blocks):
 *   trait PcaReadyGenotypeAccessor          /root/reference/src/prepare.rs:1838-2030
 *   PCA::new / rfit / transform             /root/reference/src/main.rs:602,648-660
 *   EigenSNPCoreAlgorithm::compute_pca      /root/reference/src/main.rs:359-366
 * This ABI is a PUSH model: genotypes are uploaded once (1 B or 0.25 B per genotype), stay in
 * HBM, and every pass over them runs on the device; the pull API survives as
 * gpca_standardize_block() for boundary parity.
 *
 * Threading: one handle = one GPU.  Every entry point takes the handle's (recursive) lock, so a handle may be shared
 * between host threads the way the reference shares its `Clone + Send + Sync` accessor between rayon workers
 * (prepare.rs:1770-1779, 1838): calls are serialised per handle, different handles run concurrently (one host thread may
 * drive handles on several GPUs: every entry point makes the handle's device the calling thread's current HIP device).
 * The pull API is the exception, as in the reference, whose accessor is served by 1-16 actor threads in parallel
 * (main.rs:279-283): gpca_standardize_block holds the lock only while it checks its ids, then runs its copies and its
 * kernel on one of up to 16 lanes (a stream and scratch of its own) -- calls from different threads overlap; every other
 * entry point first waits until no pull is in flight, so the matrix and its statistics never change under one.  gpca_destroy
 * must not race with other calls on the same handle; gpca_last_error() returns the calling thread's own last failure on
 * the handle (or, for a thread that has not failed on it, the handle's last message).  Functions return GPCA_OK (0) or a
 * negative gpca_status.
 *
 * Limits: k + oversample <= 128 sketch columns on GPCA_PREC_I8_EXACT (<= 64 on GPCA_PREC_F32_MFMA and in the EigenSNP stage calls: the
 * reference adds 10 to any k <= min(samples, variants), main.rs:621-628, 636); GPCA_PREC_I8_EXACT holds up to 2^22 (4 194 304) samples per matrix (i32
 * accumulators; GPCA_PREC_F32_MFMA has no such bound); SNP rows per handle are bounded by device memory only (64M rows x 1 000
 * samples and 10M x 100k as 2-bit codes were run on one MI355X), the bit-for-bit guarantees between partitions of the same
 * matrix (streamed = resident, any kernel variant) hold up to 2^25 (33.5M) rows per handle, where integer sums stay below 2^53.
 */
#ifndef GPCA_H
#define GPCA_H

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#define GPCA_API __attribute__((visibility("default")))
#else
#define GPCA_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define GPCA_VERSION 250 /* 0.2.5: a zeroed gpca_config is the fast exact path with automatic residency (the enum values of gpca_precision /
                            gpca_storage changed: 0 now means "the library's choice"); the l x l eigen step runs on the device */
#define GPCA_MISSING_I8 (-127) /* bed_reader i8 missing code, prepare.rs:1224 */

typedef struct gpca_handle gpca_handle;

typedef enum gpca_status {
    GPCA_OK = 0,
    GPCA_ERR_BAD_ARG = -1,
    GPCA_ERR_OOM = -2,
    GPCA_ERR_HIP = -3,
    GPCA_ERR_RCCL = -4,
    /* replaces the hard error of prepare.rs:1909-1911, 1961-1963, 2008-2009 */
    GPCA_ERR_MISSING_GENOTYPE = -5,
    GPCA_ERR_NOT_CONVERGED = -6, /* sketch lost rank (CholQR pivot <= 0); a null logistic fit that does not converge (a13) */
    GPCA_ERR_STATE = -7,         /* call order: e.g. rsvd before stats */
    GPCA_ERR_NO_DEVICE = -8,
    GPCA_ERR_INVALID_GENOTYPE = -9 /* a kept SNP holds a value outside {0,1,2} */
} gpca_status;

/* Arithmetic used by the two tall-skinny products.  0 -- what `gpca_config cfg = {0}`, a Rust `GpcaConfig::default()` or
 * gpca_create(NULL) give -- is the library's choice: the exact-integer path, the fastest parity-green one (a randomized PCA of 1M x 10k
 * in 10 ms against 28 ms on the f32 matrix cores). */
typedef enum gpca_precision {
    GPCA_PREC_DEFAULT = 0,  /* = GPCA_PREC_I8_EXACT */
    GPCA_PREC_I8_EXACT = 1, /* v_mfma_i32_32x32x32_i8 on fixed-point digits of the skinny operand, exact integer accumulation */
    GPCA_PREC_F32_MFMA = 2  /* v_mfma_f32_32x32x2_f32, exact f32 FMA chains (north_star's MFMA-fp32 path) */
} gpca_precision;

/* How the genotypes stay resident in HBM.  0 = GPCA_STORE_AUTO: decided when the genotypes arrive, the way both command lines decide it
 * (main.rs has no such choice: its matrix is f64): rows of >= 1 024 samples stay as 2-bit codes -- a quarter of the HBM and the faster
 * kernels there -- narrower ones as int8 (2-bit rows pad to 1 024 samples, int8 rows to 256).  An int8 upload that turns out to hold a
 * value outside {0, 1, 2, -127} is kept as int8 (2-bit codes could only store it as "missing"); panel streams cannot look ahead and
 * follow the sample count alone.  gpca_get_storage reports what was chosen. */
typedef enum gpca_storage {
    GPCA_STORE_AUTO = 0,
    GPCA_STORE_2BIT = 1, /* 0.25 B per genotype (PLINK-like packing of dosage codes), decoded in the GEMM prologues of either
                            precision.  10M SNPs x 100k samples = 250 GB: fits one MI355X. */
    GPCA_STORE_INT8 = 2  /* 1 B per genotype */
} gpca_storage;

typedef struct gpca_config {
    int32_t device;    /* HIP ordinal; -1 = current device */
    int32_t precision; /* gpca_precision */
    int32_t storage;   /* gpca_storage */
    int32_t digit_planes; /* GPCA_PREC_I8_EXACT only (3 needs an explicit GPCA_STORE_2BIT).  4: four signed base-128 digit planes of the skinny operand (28-bit fixed point per
                             column).  3: three signed base-256 planes (24-bit; exact integer accumulation as before) -- a quarter
                             less matrix-core work; implemented for GPCA_STORE_2BIT, whose kernels are matrix-core bound.
                             0 = the library's choice: 4 on int8 rows (HBM-bound), 3 on 2-bit rows (measured max|dPC| <= 3e-7 against
                             the f64 checker on every parity shape, tighter than GPCA_PREC_F32_MFMA). */
    int32_t reserved[4];  /* [0] = GPCA_CFG_* flags below (0 = the defaults); [1], [2] = resident-wave targets of the two GEMM grids (0 = the
                             values tuned on MI355X: 1 024 / 2 048; smaller values give small grids -- how the tests reach every round and
                             task pattern on small matrices); [3] must be 0.  Which kernels run is decided here, by the caller: the library
                             reads no environment variable for it. */
} gpca_config;
/* gpca_config.reserved[0] */
#define GPCA_CFG_SIMPLE_KERNELS 1 /* GPCA_PREC_I8_EXACT: the register-only reference kernels (no LDS staging, no DMA, compiler-counted waits)
                                     instead of the LDS-DMA ones: same integers, same pinned roundings -- the same bits, more slowly */
#define GPCA_CFG_NO_COMPACT 2     /* never gather the kept rows into a matrix of their own when QC drops most of them */
#define GPCA_CFG_NO_NARROW 4      /* matrices of <= 256 samples on the wide kernels (rows padded to 256 samples) */
#define GPCA_CFG_NO_SPIN_SYNC 8   /* wait for the device with hipStreamSynchronize instead of a busy-polled stream (one host core less, ~0.1 ms per call more) */
#define GPCA_CFG_ALL 15

/* SNP QC thresholds = MicroarrayDataPreparerConfig, main.rs:302-309 / prepare.rs:1281-1311,1363.
 * Effective reference defaults (clap, main.rs:545-560): 0.98 / 0.01 / 1e-6.
 * "no filtering" = {0, 0, 1.0}: only the nv==0, monomorphic (1e-9) and variance (1e-9) guards act. */
typedef struct gpca_qc_config {
    double min_snp_call_rate;   /* drop if n_valid/N <  this         prepare.rs:1283-1284 */
    double min_snp_maf;         /* drop if min(p,1-p) < this         prepare.rs:1296-1299 */
    double max_snp_hwe_p_value; /* if < 1: drop if HWE p <= this     prepare.rs:1306-1311 */
} gpca_qc_config;

/* ---- lifecycle ------------------------------------------------------------------------- */
GPCA_API int gpca_version(void);
GPCA_API const char* gpca_status_string(int status);
GPCA_API int gpca_create(const gpca_config* cfg, gpca_handle** out);
GPCA_API int gpca_destroy(gpca_handle* h);
GPCA_API const char* gpca_last_error(gpca_handle* h);

/* ---- genotype residency (replaces IoService + bed_reader reads, prepare.rs:622-629,682-693,
 *      and build_matrix's N x M f64, vcf.rs:317-345) ------------------------------------- */
/* SNP-major int8 dosages (count of allele 1: 0/1/2, -127 missing); row i at snp_major + i*ld. */
GPCA_API int gpca_upload_genotypes_i8(gpca_handle* h, const int8_t* snp_major, int64_t M, int64_t N, int64_t ld);
/* PLINK .bed payload after the 3-byte magic: M rows of ceil(N/4) bytes, 2 bits/sample LSB-first;
 * decoded on the device with count_a1 semantics (00->2, 10->1, 11->0, 01->missing). */
GPCA_API int gpca_upload_bed2bit(gpca_handle* h, const uint8_t* bed_rows, int64_t M, int64_t N);
/* Synthetic workload of SURVEY.md 8(d), generated on the device (bit-identical to
 * oracle/gpca_oracle.c:orc_synth_genotypes).  thresh: host uint32 [M][P] = floor(p*2^32). */
GPCA_API int gpca_synth_genotypes(gpca_handle* h, int64_t M, int64_t N, uint64_t seed, const uint32_t* thresh,
                         int32_t P, int64_t snp_offset);
GPCA_API int gpca_download_genotypes_i8(gpca_handle* h, int8_t* out, int64_t ld);

/* ---- g: panel sources and out-of-core streaming (BASELINE.json configs[4]; the reference never holds the matrix either:
 *      its solver pulls snp_processing_strip_size-row strips through the accessor, main.rs:322,584, prepare.rs:1839-2022) */
typedef enum gpca_panel_kind {
    GPCA_PANEL_HOST_I8 = 0,  /* `fill` writes int8 SNP-major rows (0/1/2, -127 missing), row pitch ld = N */
    GPCA_PANEL_HOST_BED = 1, /* `fill` writes PLINK .bed rows (2 bits/sample, count_a1 decode), row pitch ld = ceil(N/4) */
    GPCA_PANEL_SYNTH = 2,    /* device generator of gpca_synth_genotypes: thresh = uint32 [M][n_pop] = floor(p * 2^32) */
    GPCA_PANEL_SYNTH16 = 3,  /* fast device generator, one 16-bit uniform per genotype (SplitMix64 in counter mode): thresh = uint32 [M][n_pop],
                                high half = floor(P(g >= 1) * 65536), low half = floor(P(g = 2) * 65536); sample n belongs to
                                population (n / 16) % n_pop */
    /* The whole matrix sits in the caller's address space (malloc'ed, or a memory-mapped .bed payload: what bed_reader opens at
     * prepare.rs:622-629): `user` = address of row 0, `host_ld` = row pitch in bytes (0 = tight: N, or ceil(N/4)).  No callback:
     * the library's own copy threads move the rows of a panel into its pinned staging ring, or -- GPCA_SOURCE_REGISTER -- the
     * mapping is page-locked once at open and every panel is DMA-ed straight out of it (no staging copy at all).  The memory must
     * stay valid and unchanged until the stream is closed (gpca_stream_open) or the call returns (gpca_load_from_source). */
    GPCA_PANEL_MAPPED_I8 = 4,
    GPCA_PANEL_MAPPED_BED = 5
} gpca_panel_kind;
/* gpca_panel_source.flags */
#define GPCA_SOURCE_REGISTER 1 /* MAPPED_*: hipHostRegister the mapping at open (zero staging); if the pages cannot be locked the
                                  staged path is used instead -- gpca_stream_get_info reports which */
/* Write rows [row0, row0 + rows) of the matrix into dst (pinned host memory owned by the library).  Return 0, or
 * non-zero to abort the pass (reported as GPCA_ERR_BAD_ARG with the row range in the message).
 * Threading: called from ONE library-owned worker thread per source (never concurrently with itself), rows ascending within a
 * pass, up to staging_buffers - 1 panels ahead of the panel being copied to the device -- so the host copy of panel p + 2
 * overlaps the H2D copy of p + 1 and the GEMMs of p.  It runs while a pass (gpca_snp_stats / gpca_rsvd / gpca_transform /
 * gpca_load_from_source) is in progress on another thread, which holds the handle's lock: it may block on I/O, it must not
 * call into the same handle.  Every panel is asked exactly once per pass (cached panels once in all); after a failure no
 * further panel is asked in that pass. */
#define GPCA_SOURCE_BENCH_HOLD 2 /* SYNTH16, MEASUREMENT ONLY: a ring / cache buffer that already holds a generated panel of the same height is not
                                   generated again -- every pass then multiplies whatever panels the buffers held first.  The numbers a call
                                   returns are NOT a PCA of the source; what it measures is the engine's rate over streamed panels with the
                                   generator out of the way (bench.py: config5_per_gpu_shard_streamed.engine_rate_with_fills_hidden). */
typedef int (*gpca_panel_fn)(void* user, int64_t row0, int64_t rows, void* dst, int64_t ld);
typedef struct gpca_panel_source {
    int32_t kind;           /* gpca_panel_kind */
    int32_t n_pop;          /* SYNTH*: populations (columns of thresh) */
    gpca_panel_fn fill;     /* HOST_*: the callback above */
    void* user;             /* HOST_*: passed to fill; MAPPED_*: address of row 0 */
    const uint32_t* thresh; /* SYNTH*: host table, copied to the device at open */
    uint64_t seed;          /* SYNTH* */
    int64_t snp_offset;     /* SYNTH*: global index of row 0 (row shards of one matrix draw the rows they would unsharded) */
    int64_t host_ld;        /* MAPPED_*: row pitch in bytes (0 = tight) */
    int64_t flags;          /* GPCA_SOURCE_* */
} gpca_panel_source;
/* Resident load through a panel source (chunked through bounded staging: a 250 GB .bed needs no second device copy). */
GPCA_API int gpca_load_from_source(gpca_handle* h, const gpca_panel_source* src, int64_t M, int64_t N);
/* Out-of-core mode: the matrix is never resident.  Every pass of gpca_snp_stats / gpca_rsvd / gpca_transform walks
 * ceil(M / panel_rows) panels through a ring of `ring_slots` (>= 2) HBM panel buffers; panel p + 1 is generated or
 * copied on a second stream while panel p is multiplied.  panel_rows is rounded up to a multiple of 128; 0 picks
 * 131 072 rows (a full grid of the row-parallel GEMM) or as many as fit the ring in half of the free HBM (host sources: at most
 * 2 GiB of pinned host staging per panel, three staging panels -- GPCA_STAGE_BUFFERS=2..8).  Requires GPCA_PREC_I8_EXACT (either storage).  With gpca_stream_set_fused(h, 0) the
 * results are bit-identical to the resident engine on the same matrix; the default (fused) form is described below.  The pull API
 * (gpca_standardize_block) and gpca_download_genotypes_i8 need a resident matrix. */
GPCA_API int gpca_stream_open(gpca_handle* h, const gpca_panel_source* src, int64_t M, int64_t N, int64_t panel_rows,
                              int32_t ring_slots);
/* fused = 1 (the default after gpca_stream_open): a power iteration reads every panel ONCE -- G Q, quantisation and G^T T per panel
 * while it sits in HBM -- so gpca_rsvd makes 2 + power_iters passes over the source instead of 2 + 2 * power_iters (4 instead of 6
 * at q = 2: what counts when the source is a disk or the host link).  Every panel then quantises its rows against its own column
 * maxima: results differ from the resident engine at the 1e-9 level of the 28-bit fixed point (as a row-sharded run does).
 * fused = 0: the 6-pass form, bit-identical to the resident engine. */
GPCA_API int gpca_stream_set_fused(gpca_handle* h, int32_t fused);
/* Panel cache: HBM the ring and the solver's workspace leave free holds the LEADING panels for good -- each is asked of the
 * source once (normally during gpca_snp_stats) and read in place on every later pass, so a matrix 3x the HBM costs 2/3 of the
 * source traffic per pass, and one that fits is read once.  max_bytes: upper bound for the cache (whole panels are taken);
 * < 0 = all free device memory less the solver's workspace estimate and a 4 GiB margin; 0 drops the cache.  The source must
 * return the same rows every time it is asked (it must anyway: every pass re-reads it).  Results do not change.
 * *n_cached (may be NULL) receives the number of cached panels.  GPCA_ERR_OOM keeps the panels allocated so far. */
GPCA_API int gpca_stream_set_cache(gpca_handle* h, int64_t max_bytes, int32_t* n_cached);
/* What the open panel stream looks like, and where its time went since gpca_stream_open (host-side, always collected). */
typedef struct gpca_stream_info {
    int64_t panel_rows;
    int32_t n_panels, ring_slots, n_cached;
    int32_t staging_buffers; /* pinned host staging panels (0: device generator, or zero-staging) */
    int32_t zero_staging;    /* 1 = MAPPED_* source page-locked in place, panels DMA-ed straight from the caller's memory */
    int32_t copy_threads;    /* MAPPED_* staged: threads that copy a panel into staging */
    int64_t fills;           /* panels asked of the source so far */
    double fill_host_ms;     /* host time spent producing panels into staging (callback / copy threads), summed over the worker's jobs */
    double fill_wait_ms;     /* time the pass thread was blocked on the staging ring (panel not staged yet, or every buffer still in flight on
                                the link): compare with fill_host_ms to tell a slow source from a saturated link */
    double register_ms;      /* hipHostRegister at open (zero-staging) */
    int64_t reserved[4];
} gpca_stream_info;
GPCA_API int gpca_stream_get_info(gpca_handle* h, gpca_stream_info* out);
GPCA_API int gpca_dims(gpca_handle* h, int64_t* M, int64_t* N);
/* The residency in use (GPCA_STORE_INT8 / GPCA_STORE_2BIT; GPCA_STORE_AUTO until the first genotypes have arrived) and the precision. */
GPCA_API int gpca_get_storage(gpca_handle* h, int32_t* storage, int32_t* precision);
/* Free and total memory of the handle's device in bytes (hipMemGetInfo): what a host needs to choose between a resident load
 * (M x N bytes int8, M x N / 4 packed, plus about 1 KiB per SNP row and 8 KiB per sample of workspace) and gpca_stream_open. */
GPCA_API int gpca_get_device_memory(gpca_handle* h, int64_t* free_bytes, int64_t* total_bytes);

/* ---- a1/a3: SNP QC + standardisation parameters (prepare.rs:1100-1422, 1641-1745) -------- */
/* Any of mu/sigma/keep may be NULL.  mu, sigma are the f32 values the reference stores
 * (prepare.rs:1313,1364); 0 for dropped SNPs. */
GPCA_API int gpca_snp_stats(gpca_handle* h, const gpca_qc_config* qc, float* mu, float* sigma, uint8_t* keep);
/* counts[i] = {n_valid, n_hom0, n_het, n_hom2}; reason[i]: 0 kept, 1 call-rate, 2 no valid,
 * 3 MAF, 4 monomorphic, 5 HWE, 6 variance.  Either may be NULL. */
GPCA_API int gpca_get_snp_qc_detail(gpca_handle* h, uint32_t* counts, uint8_t* reason);
/* Caller-supplied parameters instead of gpca_snp_stats (e.g. LD-block restriction via keep). */
GPCA_API int gpca_set_standardization(gpca_handle* h, const float* mu, const float* sigma, const uint8_t* keep);
/* Current parameters, length M each (any may be NULL): what gpca_snp_stats computed or gpca_set_standardization set. */
GPCA_API int gpca_get_standardization(gpca_handle* h, float* mu, float* sigma, uint8_t* keep);
/* Host helper (no GPU): a symmetric eigen-solver (Householder tridiagonalisation + implicit QL) -- what gpca_rsvd ran for its l x l
 * step on the host up to round 4, kept as the pin of the device solver: CPU-only tests hold it to LAPACK, GPU tests hold the device
 * solver to it.  a_sym: n x n row-major (n <= 128); w: eigenvalues descending; v: eigenvectors in columns, row-major. */
GPCA_API int gpca_host_eigh_desc(const double* a_sym, int32_t n, double* w, double* v);
/* Test hook (GPU): the DEVICE eigen-solver gpca_rsvd runs for its l x l step (csrc/small_eig.hip: cyclic two-sided Jacobi in LDS up to
 * 64 columns, tridiagonalisation + QL split over waves for 65-128; the call's stream never waits for the host), on a caller's matrix;
 * same conventions as above. */
GPCA_API int gpca_device_eigh_desc(gpca_handle* h, const double* a_sym, int32_t n, double* w, double* v);
/* Test hook (GPU): the orthonormalisation gpca_rsvd runs between its GEMM sweeps (CholeskyQR, `rounds` = 1 or 2: Gram, Cholesky +
 * inverse, right-multiplication, s = Q^T 1) on a caller's sketch Y [N][l], through the product's own stage function and with the
 * handle's sample mask.  The handle holds genotypes and standardisation (N = its sample count); l <= min(N, PCA SNPs), l <= 128
 * (64 on GPCA_PREC_F32_MFMA).  Q [N][l]: the basis; s [l] (may be NULL): its column sums; *pivot_flag: the device's pivot flag
 * (j + 1 for the first pivot j that was not finite, else 0), returned as data -- the hook itself returns GPCA_OK.  The results of an
 * earlier gpca_rsvd are gone afterwards. */
GPCA_API int gpca_device_orth(gpca_handle* h, const double* Y, int32_t l, int32_t rounds, double* Q, double* s, int32_t* pivot_flag);
/* Test hook (GPU): the tail of a call -- Gram, the l x l eigen step, scores with the sign rule, loadings, the verdict on the result
 * block -- on a caller's factors Q [N][l] (f64, any matrix) and B [M][l] (f32; only PCA SNP rows are read), through the function
 * gpca_rsvd and gpca_refine share.  zmode 0 (step 4 of gpca_rsvd): B^T B = V diag(w) V^T, scores = Q V_k diag(sv), loadings =
 * B V_k diag(1 / sv) (0 where sv = 0); zmode 1 (the tail of gpca_refine): Q^T Q = V diag(w) V^T, scores = Q V_k, loadings = B V_k.
 * Results through the getters (scores, singular values [l], eigenvalues = w / (samples - 1), loadings). */
GPCA_API int gpca_device_tail(gpca_handle* h, const double* Q, const float* B, int32_t l, int32_t k, int32_t zmode);
/* Test hook (GPU): the sketch Y = A^T Omega that opens gpca_rsvd(h, l, 0, .., seed) -- Omega into T' = r o Omega and c = b^T Omega (on
 * GPCA_PREC_I8_EXACT straight into digit planes against the analytic column bound), the fold of c, K2 -- through the product's own
 * stage functions and before any exchange: Y [N][l] is the rank-local result.  Runs on the compact child of the kept rows whenever
 * gpca_rsvd would (*on_child = 1, else 0).  Resident and streamed handles, both precisions; a handle with an all-reduce hook is
 * accepted (that is how a handle gets its snp_offset) and the hook is not called.  The results of an earlier gpca_rsvd are gone
 * afterwards. */
GPCA_API int gpca_device_sketch(gpca_handle* h, int32_t l, uint64_t seed, double* Y, int32_t* on_child);
/* Test hook (GPU): one power iteration of gpca_rsvd on a caller's sketch Yin [N][l]: CholeskyQR2 (two rounds), then Y = A^T (A Q) as
 * gpca_rsvd chooses it for this handle -- the fused one-read sweep on a streamed handle unless gpca_stream_set_fused(h, 0), otherwise
 * K1 over all rows followed by K2 -- on the handle's own matrix (never the compact child).  Q [N][l]: the f64 basis; Tq [M][l]: T' =
 * r o (A Q) in f32 as K2 reads it (rows QC dropped are zero); c [l]: b^T (A Q); Yout [N][l]: the new sketch.  Needs an unsharded handle on
 * GPCA_PREC_I8_EXACT (GPCA_ERR_STATE otherwise: the f32 path keeps T' blocked, not row-major).
 * The results of an earlier gpca_rsvd are gone afterwards. */
GPCA_API int gpca_device_power(gpca_handle* h, const double* Yin, int32_t l, double* Q, float* Tq, double* c, double* Yout);
/* Host helper, same branches as prepare.rs:1641-1745. */
GPCA_API double gpca_hwe_chi_squared_p_value(uint64_t n_hom1, uint64_t n_het, uint64_t n_hom2);

/* ---- a2/a7: the pull API (prepare.rs:1838-2030) ------------------------------------------ */
/* PcaSnpId = rank among kept SNPs; QcSampleId = sample column.  out: f32 [ns][nj], C order.
 * Returns GPCA_ERR_MISSING_GENOTYPE if any requested genotype is -127 (message names the ids). */
GPCA_API int gpca_standardize_block(gpca_handle* h, const int64_t* pca_snp_ids, int64_t ns,
                           const int64_t* qc_sample_ids, int64_t nj, float* out);
GPCA_API int64_t gpca_num_pca_snps(gpca_handle* h);   /* prepare.rs:2024-2026 */
GPCA_API int64_t gpca_num_qc_samples(gpca_handle* h); /* prepare.rs:2027-2029 */
/* original row (BIM index) of every PCA SNP, length gpca_num_pca_snps; prepare.rs:1833-1835 */
GPCA_API int gpca_get_pca_snp_rows(gpca_handle* h, int64_t* rows);

/* ---- a5/a6: randomized PCA (PCA::rfit main.rs:648-656; compute_pca main.rs:365) ---------- */
/* l = k + oversample columns (<= 128, see Limits); power_iters QR-stabilised iterations; Omega from
 * Philox4x32-10 keyed by seed.  Requires stats.  Results stay on the device until fetched.
 * Row-sharded runs (gpca_comm_init / gpca_set_allreduce_hook): the ranks agree on a status word before the first and after
 * the last exchange of the call, so a rank-local failure (missing genotype in one shard, out of memory, a failed launch)
 * is returned by EVERY rank instead of leaving the others inside a collective. */
GPCA_API int gpca_rsvd(gpca_handle* h, int32_t k, int32_t oversample, int32_t power_iters, uint64_t seed);
GPCA_API int gpca_get_scores(gpca_handle* h, float* out /* [N][k] */);       /* main.rs:389 */
GPCA_API int gpca_get_scores_f64(gpca_handle* h, double* out /* [N][k] */);  /* main.rs:659 (f64 path) */
GPCA_API int gpca_get_eigenvalues(gpca_handle* h, double* out /* [k] */);    /* main.rs:394 */
GPCA_API int gpca_get_singular_values(gpca_handle* h, double* out /* [k+oversample] */);
GPCA_API int gpca_get_loadings(gpca_handle* h, float* out /* [num_pca_snps][k] */); /* main.rs:407 */
/* PCA::transform (main.rs:659) on the resident matrix: scores = A^T * loadings, f64 [N][k]. */
GPCA_API int gpca_transform(gpca_handle* h, double* out);
/* ---- a7: projection of this handle's genotypes onto a fitted model (PCA::transform(x) of efficient_pca on new samples, main.rs:659):
 * mu, sigma: f32 [M]; W: f32 [M][k] row-major in THIS handle's row order, zero rows = not in the model; scores: f64 [N][k];
 * n_used: int32 [N] or NULL (model rows with an observed call).  Missing calls are mean-imputed: their standardised value is 0.
 * Needs genotypes only (no gpca_snp_stats / gpca_rsvd) and leaves every fitted result of the handle as it was.  1 <= k <= 128.
 * A model row with a non-finite mu / sigma / W entry or sigma <= 0 is GPCA_ERR_BAD_ARG (the message names the row); a model row
 * holding a value outside {0, 1, 2, missing} is GPCA_ERR_INVALID_GENOTYPE.  GPCA_PREC_F32_MFMA handles return GPCA_ERR_STATE.
 * With the handle's own model (loadings scattered to gpca_get_pca_snp_rows, mu / sigma of gpca_get_standardization) and no missing
 * call in a model row, the scores equal gpca_transform's bit for bit -- as long as gpca_rsvd ran on the handle's own rows.  When QC
 * dropped so many rows that gpca_rsvd ran on a compacted copy of the kept rows (at least 32 Ki rows and 8 MiB dropped, at most half
 * of the rows kept), gpca_transform sums c = b^T W over other 64-row groups and the two may differ in the last bits.  Row-sharded handles: every rank passes its own rows' model;
 * scores and counts are summed in one exchange that also carries the status word, so a rank-local failure comes back from every rank. */
GPCA_API int gpca_project(gpca_handle* h, const float* mu, const float* sigma, const float* W, int32_t k, double* scores, int32_t* n_used);

/* ---- a8: genetic relationship matrix of this handle's kept rows (the reference's exact-PCA check, tests/pca.py: GRM = X X^T / kept).
 * Z[i][n] = r_i g + b_i for an observed call (GPCA_GRM_STANDARDIZED: the matrix gpca_rsvd factorises, r = 1 / sigma, b = -mu r in f32 as
 * gpca_set_standardization makes them) or g - mu_i (GPCA_GRM_CENTRED), and 0 for a missing call.  Over the kept rows, K of them summed
 * over all ranks:  grm[j][k] = (1 / K) sum_i Z[i][j] Z[i][k];  npairs[j][k] = kept rows where both j and k are observed (exact).
 * Writes rows row0 <= j < row1 of the lower triangle, diagonal included, packed row-major: element (j, k <= j) at
 * j (j + 1) / 2 - row0 (row0 + 1) / 2 + k (GCTA's .grm.bin order), so a band is bit-identical to the same rows of the full call.
 * npairs may be NULL.  Works on every handle (int8 or 2-bit, resident or streamed, either precision, sharded); the sample mask is
 * ignored and no fitted result of the handle is touched.  Sharded handles: every rank passes the same band; bands and status go
 * through the exchange, so a rank-local failure comes back from every rank.  Errors: GPCA_ERR_BAD_ARG (scaling, row range, a kept
 * row with a negative or non-finite mean), GPCA_ERR_STATE (no standardisation, or K = 0), GPCA_ERR_INVALID_GENOTYPE (a kept row holds
 * a value outside {0, 1, 2, missing}), GPCA_ERR_OOM (the band does not fit in device memory: checked before any allocation). */
enum { GPCA_GRM_STANDARDIZED = 0, GPCA_GRM_CENTRED = 1 };
GPCA_API int gpca_grm(gpca_handle* h, int32_t scaling, int64_t row0, int64_t row1, double* grm, float* npairs /* may be NULL */);

/* ---- a9: KING-robust kinship of this handle's kept rows (relatedness that needs no allele frequencies: plink2 --make-king).
 * Per sample and kept row: H = [g == 1], M = [missing], X = g - 1 for g in {0, 2} (0 otherwise).  Over the K kept rows (all ranks):
 *   HETHET = sum H_a H_b;  NSNP = K - miss_a - miss_b + sum M_a M_b;  het_ab = het_a - sum H_a M_b;  het_ba = het_b - sum M_a H_b
 *   (het_x, miss_x: the sample's het and missing counts);  homhom = NSNP - het_ab - het_ba + HETHET;  IBS0 = (homhom - sum X_a X_b) / 2
 *   kinship = 0.5 - (4 IBS0 + het_ab + het_ba - 2 HETHET) / (4 min(het_ab, het_ba)),  NaN when min(het_ab, het_ba) = 0.
 * Every count is an exact integer; the kinship is computed in f64 from them, so only the division and the last subtraction round.
 * Writes rows row0 <= j < row1 of the STRICTLY lower triangle packed row-major: pair (j, k < j) at j (j - 1) / 2 - row0 (row0 - 1) / 2 + k,
 * so a band is bit-identical to the same rows of the full call.  counts (may be NULL): [pairs][3] = NSNP, HETHET, IBS0.  Works on every
 * handle (int8 or 2-bit, resident or streamed, either precision, sharded); the sample mask is ignored and no fitted result is touched.
 * Sharded handles: every rank passes the same band; the integer counts, K and the status word are summed in one exchange and the
 * kinship is computed after it, so a rank-local failure comes back from every rank and two ranks give the one-rank bits.
 * Errors: GPCA_ERR_STATE (no standardisation, or K = 0), GPCA_ERR_BAD_ARG (row range, or K >= 2^31), GPCA_ERR_INVALID_GENOTYPE (a kept
 * row holds a value outside {0, 1, 2, missing}), GPCA_ERR_OOM (the band does not fit in device memory: checked before any allocation). */
GPCA_API int gpca_king(gpca_handle* h, int64_t row0, int64_t row1, double* kinship, int32_t* counts /* [pairs][3]; may be NULL */);

/* ---- a10: windowed LD of this handle's kept rows: the unphased r^2 of plink's --indep-pairwise, SNP against the SNPs after it.
 * Rows are addressed in PCA-SNP order (i = rank among the kept rows, the ids of gpca_standardize_block / gpca_get_pca_snp_rows;
 * K = gpca_num_pca_snps), so windows are counted over the SNPs the run keeps.  Row i = row0 + t is paired with every j,
 * i < j < win_end[t]; the pair's slot is d = j - i - 1.  Required: 0 <= row0 <= row1 <= K, wmax >= 1,
 * i + 1 <= win_end[t] <= min(K, i + 1 + wmax): one primitive serves windows of a variant count, windows in kb (ragged) and chromosome
 * boundaries (the last row of a chromosome has an empty window).  Per pair and sample, with o = [call observed] and g' = g on an
 * observed call, 0 on a missing one:
 *   n = sum o_i o_j,  sx = sum g'_i o_j,  sy = sum o_i g'_j,  sxx = sum g'_i^2 o_j,  syy = sum o_i g'_j^2,  sxy = sum g'_i g'_j
 *   cov = n sxy - sx sy,  vx = n sxx - sx sx,  vy = n syy - sy sy   (exact integers in f64)
 *   r2 = (cov cov) / (vx vy) in f64: exactly these two products and one division;  NaN when vx <= 0 or vy <= 0
 * -- the squared Pearson correlation of the two dosage vectors over the samples observed at both SNPs.
 * r2 [rows][wmax];  counts [rows][wmax][6] = n, sx, sy, sxx, syy, sxy;  above [rows][ceil(wmax / 64)]: bit d % 64 of word d / 64 =
 * (r2 > threshold), NaN is not above, from the same f64 value r2 receives.  Slots outside a row's window are 0 in all three, padding
 * bits included.  Any of the three may be NULL, not all; threshold is read only with above and must be finite then.
 * A row band is bit-identical to the same rows of a wider call, int8 and 2-bit residency give the same bits, and so does a
 * GPCA_PREC_F32_MFMA handle (the call reads only the genotypes and the keep mask); the sample mask is ignored and no fitted result
 * of the handle is touched.
 * Out of scope: streamed and row-sharded handles (a window crosses panel and shard boundaries and needs a halo of wmax rows): they
 * return GPCA_ERR_STATE.  No r^2 table file, no phased r^2 / D'.
 * Errors: GPCA_ERR_STATE (no standardisation, K = 0, a streamed handle, a row-sharded handle), GPCA_ERR_BAD_ARG (ranges, win_end,
 * wmax, all outputs NULL, a non-finite threshold, 4 N >= 2^31), GPCA_ERR_INVALID_GENOTYPE (a row the call reads holds a value outside
 * {0, 1, 2, missing}; the message names the row), GPCA_ERR_OOM (the band's buffers do not fit in device memory: checked before any
 * allocation). */
GPCA_API int gpca_ld_window(gpca_handle* h, int64_t row0, int64_t row1, const int64_t* win_end /* [row1 - row0] */, int32_t wmax,
                            double threshold, double* r2 /* [rows][wmax] */, int32_t* counts /* [rows][wmax][6] */,
                            uint64_t* above /* [rows][ceil(wmax / 64)] */);

/* ---- a11: PC-Relate (Conomos et al. 2016): kinship and inbreeding with the ancestry taken out, from this handle's kept rows (K of
 * them, in PCA-SNP order) and P <= 32 caller-supplied sample coordinates V [N][P] (f64; normally the fitted or projected scores).
 * train [N] (NULL = everyone): the samples the regression is fitted on (normally the KING in-set).  g = the call, o = [observed].
 *  1. design and hat matrix (host, f64): x_n = (1, V_n1 / c_1, ..., V_nP / c_P), c_j = the root mean square of column j over the
 *     training samples; H = (X^T X)^-1 X^T over the training samples by Cholesky, 0 for the other samples.
 *  2. beta_i = sum_train H_n g'_in + mbar_i sum_train H_n (1 - o_in), mbar_i = the mean of row i's observed training calls (missing
 *     training calls are imputed to it); accumulated in f64, rounded once to f32, [K][P + 1].  A row with no observed training call
 *     gets beta = 0 and every entry of it is invalid.
 *  3. mu_in = 0.5f * (fmaf chain over j = 0 .. P of beta_ij * (float)x_nj, from 0), in f32;  valid_in = o_in and tau_f < mu_in and
 *     mu_in < 1.0f - tau_f, tau_f = (float)tau.  P = 0: mu_in = mbar_i / 2, the homogeneous estimator.
 *  4. r = valid (g - 2 mu), s = valid sqrt(mu (1 - mu)) in f32;  num_ab = sum_i r_ia r_ib, den_ab = sum_i s_ia s_ib on
 *     v_mfma_f32_32x32x2_f32 (bit for bit an fmaf chain over the kept rows), flushed to f64 running sums every 256 kept rows counted
 *     from the first;  nsnp_ab = sum_i valid_ia valid_ib (exact);  kinship_ab = num_ab / (4 den_ab) in f64, NaN when nsnp_ab = 0.
 *     The diagonal is the self-kinship (1 + F_a) / 2.
 * gpca_pcrelate_isaf: mu [rows][N] and / or beta [rows][P + 1] of kept rows [row0, row1), 0 <= row0 <= row1 <= K (either may be NULL,
 *   not both).  gpca_pcrelate: rows row0 <= a < row1 of the lower triangle WITH the diagonal in gpca_grm's packing: element (a, b <= a)
 *   at a (a + 1) / 2 - row0 (row0 + 1) / 2 + b; nsnp (may be NULL) in the same packing.  0 <= tau < 0.5.
 * A band is bit-identical to the same rows of the full call; int8 and 2-bit residency give the same bits, and so does a
 * GPCA_PREC_F32_MFMA handle (the calls read only the genotypes and the keep mask); the sample mask is ignored and no fitted result is
 * touched.  Out of scope: the small-sample scale correction of GENESIS, the k0 / k2 IBD-sharing estimates, and streamed and
 * row-sharded handles (the f32 / f64 sums are not associative across panels or ranks): GPCA_ERR_STATE.
 * Errors: GPCA_ERR_STATE (no standardisation, K = 0, a streamed handle, a row-sharded handle), GPCA_ERR_BAD_ARG (P outside [0, 32],
 * fewer than P + 2 training samples, a non-finite V entry, a zero or collinear column of V on the training samples, tau, the row
 * range, K >= 2^31), GPCA_ERR_INVALID_GENOTYPE (a kept row holds a value outside {0, 1, 2, missing}; the message names the row),
 * GPCA_ERR_OOM (the band and the regression's workspace do not fit in device memory: checked before any allocation). */
GPCA_API int gpca_pcrelate_isaf(gpca_handle* h, const double* V /* [N][P] */, int32_t P, const uint8_t* train /* [N] or NULL */, int64_t row0,
                                int64_t row1, float* mu /* [rows][N] or NULL */, float* beta /* [rows][P + 1] or NULL */);
GPCA_API int gpca_pcrelate(gpca_handle* h, const double* V /* [N][P] */, int32_t P, const uint8_t* train /* [N] or NULL */, double tau,
                           int64_t row0, int64_t row1, double* kinship, int32_t* nsnp /* may be NULL */);

/* ---- a12: linear association scan: ordinary least squares of each of T traits on (1, C, g) for every kept row g of the band
 * [row0, row1), 0 <= row0 <= row1 <= K (PCA-SNP order), T >= 1, Pc >= 0, T + Pc <= 64.  It is plink's --glm on a quantitative trait,
 * except that a missing call is imputed to the row's mean over the included samples (as BOLT, regenie and fastGWA do; plink drops the
 * sample for that variant, so plink's output is claimed only for rows with no missing call among the included samples).
 *  1. host, f64, once per call: S = the included samples (include [N], NULL = everyone), n = |S|; Q [N][Pc] = an orthonormal basis of
 *     the columns of C centred over S (Cholesky of the centred columns scaled to unit norm), 0 outside S; Y~ = Y centred over S minus
 *     Q Q^T Y, 0 outside S; yy_t = |Y~_t|^2; B = [Y~ | Q], rounded once to f32; df = n - Pc - 2.
 *  2. device, one read of the genotypes: o = [observed and in S], g' = g o; n_obs = sum o, s1 = sum g', s2 = sum g'^2 (exact);
 *     d_ij = sum_n g'_in B_nj and e_ij = sum_n [missing and in S]_in B_nj on v_mfma_f32_32x32x2_f32 (the operand is the call as f32, so
 *     every product is exact), an f32 accumulator never sums more than 256 samples (groups counted from sample 0) before it is added
 *     to an f64 running sum; no split of the sample axis and no atomics.
 *  3. f64, no fused multiply-add: mbar = s1 / n_obs; xb_ij = d_ij + mbar e_ij; xx = s2 - s1 mbar; sxx = xx - sum_{j >= T} xb_ij^2 (j
 *     ascending); per trait beta = xb_it / sxx, rss = yy_t - xb_it beta, se = sqrt(rss / df / sxx), t = beta / se; a1_freq = mbar / 2.
 *     beta, se, t are NaN when n_obs = 0, xx <= 0, sxx max_vif < xx (plink's --vif rule) or rss <= 0.
 * stats [rows][T][3] = beta, se, t; xb [rows][T + Pc]; rowinfo [rows][4] = n_obs, a1_freq, xx, sxx: each may be NULL, not all three.
 * A band is bit-identical to the same rows of the full call; int8 and 2-bit residency give the same bits, and so does a
 * GPCA_PREC_F32_MFMA handle (the call reads only the genotypes and the keep mask); the sample mask is ignored and no fitted result is
 * touched.  Out of scope: case / control traits (a13 has their score test), per-variant dropping of samples, per-trait sample sets,
 * mixed models, and streamed and row-sharded handles: GPCA_ERR_STATE.
 * Errors: GPCA_ERR_STATE (no standardisation, K = 0, a streamed handle, a row-sharded handle), GPCA_ERR_BAD_ARG (T, Pc or the row
 * range out of bounds, all outputs NULL, a non-finite entry of Y or C on an included sample, df < 1, a column of C that is constant or
 * collinear over S, a trait with yy_t = 0, max_vif < 1 or not finite), GPCA_ERR_INVALID_GENOTYPE (a row the call reads holds a value
 * outside {0, 1, 2, missing}; the message names the row), GPCA_ERR_OOM (checked before any allocation). */
GPCA_API int gpca_assoc_linear(gpca_handle* h, const double* Y /* [N][T] */, int32_t T, const double* C /* [N][Pc] or NULL */, int32_t Pc,
                               const uint8_t* include /* [N] or NULL */, double max_vif, int64_t row0, int64_t row1,
                               double* stats /* [rows][T][3] or NULL */, double* xb /* [rows][T + Pc] or NULL */,
                               double* rowinfo /* [rows][4] or NULL */);
/* -log10 of the two-sided p-value of a Student t statistic with df degrees of freedom; host only, in log space (a p below 1e-308
 * does not underflow).  NaN for a NaN t or df <= 0. */
GPCA_API double gpca_student_t_log10p(double t, double df);

/* ---- a13: logistic score scan: the score test of each of T case / control traits (Y in {0, 1}) for every kept row g of the band
 * [row0, row1), the null model logit P(y = 1) = (1, C) alpha fitted once per trait and no SNP refitted: regenie step 2 --bt without
 * --firth / --spa, SAIGE without SPA, fastGWA-GLMM without the random effect.  T >= 1, Pc >= 0, T (Pc + 3) <= 64.  A missing call is
 * imputed to the row's mean over the included samples, as in a12.
 *  1. host, f64, gpca_logistic_null: S = the included samples, n = |S|; X = (1, the columns of C centred over S and scaled to unit
 *     norm: a12's standardisation and constant-column test).  Newton from alpha = (logit(ybar), 0, ...): mu = 1 / (1 + exp(-X alpha)),
 *     w = mu (1 - mu), (X^T W X) delta = X^T (y - mu) by Cholesky, alpha += delta, until max |delta| <= 1e-10 (1 + max |alpha|); mu is
 *     recomputed from the final alpha.  alpha [Pc + 1] is in the coordinates of X; mu [N] is 0 outside S.
 *     GPCA_ERR_BAD_ARG: y outside {0, 1} or not finite on S, only one class, n - Pc - 1 < 1, a non-finite entry of C on S, a constant
 *     column, a Cholesky pivot below 1e-10 of its diagonal entry (collinear).  GPCA_ERR_NOT_CONVERGED: 25 steps, or some
 *     |X alpha| > 30 (separation).  Host only, no handle, no message.
 *  2. host, f64, per trait t: r_t = y - mu, w_t = mu (1 - mu), A_t,j (j = 0 .. Pc) = the columns of W X L^-T with X^T W X = L L^T
 *     (column 0 is the intercept's); Pc + 3 columns, each rounded once to f32 and 0 outside S: the panel B.
 *  3. device: o = [observed and in S], m = [missing and in S]; the exact integers n_obs = sum o, s1 = sum g o, s2 = sum g^2 o.  A row is
 *     FLIPPED iff s1 > n_obs (its A1 mean is above 1).  The operand is x = g o on a plain row and (2 - g) o on a flipped one.
 *     d_c = sum_n x_n B_nc, e_c = sum_n m_n B_nc, q_t = sum_n x_n^2 w_t,n on v_mfma_f32_32x32x2_f32 (x, m, x^2 are 0, 1, 2, 4: every
 *     product is exact), an f32 accumulator never sums more than 256 samples (groups counted from sample 0) before it is added to an
 *     f64 running sum; no split of the sample axis and no atomics on sums.
 *  4. f64, no fused multiply-add: xbar = (s1 or 2 n_obs - s1) / n_obs, the operand's mean; U_t = d[r_t] + xbar e[r_t];
 *     a_t,j = d[A_t,j] + xbar e[A_t,j]; gwg_t = q_t + (xbar xbar) e[w_t]; vw = gwg - a_0^2; V = vw - sum_{j = 1 .. Pc} a_j^2 (j
 *     ascending); s = -1 on a flipped row, else +1; beta = s U / V, se = 1 / sqrt(V), z = s U / sqrt(V) (all for allele A1);
 *     a1_freq = (s1 / n_obs) / 2; xx = s2 - s1 (s1 / n_obs).  beta, se, z are NaN when n_obs = 0, xx <= 0, !(V > 0) or
 *     V max_vif < vw.  (V is the same in either coding; the flip keeps the cancellation in gwg - a_0^2 near a factor 3, against about
 *     200 at an A1 frequency of 0.99.)
 * stats [rows][T][5] = beta, se, z, vw, V; ua [rows][T][Pc + 3] = U, gwg, a_0 .. a_Pc in the operand's coding; rowinfo [rows][5] =
 * n_obs, a1_freq, xx, flipped (0 / 1), 0: each may be NULL, not all three.  The null fits run inside the call through the function
 * behind gpca_logistic_null; a failure returns its status and names the trait in gpca_last_error.
 * A band is bit-identical to the same rows of the full call; int8 and 2-bit residency give the same bits, and so does a
 * GPCA_PREC_F32_MFMA handle; the sample mask is ignored and no fitted result is touched.  Out of scope (a14 has the saddle-point correction, a15 the
 * approximate Firth correction): a Wald / IRLS fit per SNP, per-variant dropping of samples, case / control frequency columns (a17 counts them), mixed
 * models, and streamed and row-sharded handles: GPCA_ERR_STATE.
 * Errors: GPCA_ERR_STATE (no standardisation, K = 0, a streamed handle, a row-sharded handle), GPCA_ERR_BAD_ARG (T, Pc or the row range
 * out of bounds, all outputs NULL, max_vif < 1 or not finite, and those of step 1), GPCA_ERR_NOT_CONVERGED (step 1),
 * GPCA_ERR_INVALID_GENOTYPE (a row the call reads holds a value outside {0, 1, 2, missing}; the message names the row), GPCA_ERR_OOM
 * (checked before any allocation). */
GPCA_API int gpca_logistic_null(const double* y /* [N] */, const double* C /* [N][Pc] or NULL */, int32_t Pc,
                                const uint8_t* include /* [N] or NULL */, int64_t N, double* alpha /* [Pc + 1] */,
                                double* mu /* [N], 0 outside S */, int32_t* iters /* may be NULL */);
GPCA_API int gpca_assoc_logistic_score(gpca_handle* h, const double* Y /* [N][T], 0 / 1 */, int32_t T, const double* C /* [N][Pc] or NULL */,
                                       int32_t Pc, const uint8_t* include /* [N] or NULL */, double max_vif, int64_t row0, int64_t row1,
                                       double* stats /* [rows][T][5] or NULL */, double* ua /* [rows][T][Pc + 3] or NULL */,
                                       double* rowinfo /* [rows][5] or NULL */);
/* -log10 of the two-sided p-value of a standard normal statistic, -log10(2 Phi(-|z|)); host only, in log space (a p below 1e-308 does
 * not underflow).  NaN for a NaN z. */
GPCA_API double gpca_normal_log10p(double z);

/* ---- a14: the saddle-point correction of the logistic score scan (SPA: Dey et al. 2017, SAIGE's Saddle_Prob, regenie --spa): the
 * p-value of a13's U_t from the cumulant function of U under the null instead of the normal approximation of U / sqrt(V), which is
 * wrong by many decades for a rare variant in an unbalanced trait.  gpca_assoc_logistic_spa is gpca_assoc_logistic_score (the same
 * path: stats, ua and rowinfo carry the same bits) followed by the correction of the items (row, trait) with |z| >= spa_z.
 *  Setting.  For trait t and kept row i, in the operand's coding of a13 (a flipped row stays flipped; the two-sided p does not change
 *     under the flip): x~_n = x_n where the call is observed and in S, xbar where it is missing and in S, 0 outside S;
 *     g~_n = x~_n - sum_{j = 0 .. Pc} a_t,j Z_t,n,j (j ascending), Z_t = X L_t^-T with X and L_t of a13 steps 1 - 2: N x (Pc + 1), f64,
 *     0 outside S, built on the host beside the f32 panel; a_t,j = the values of a13 step 4, the ones ua reports.  Then X^T W g~ = 0
 *     and g~^T W g~ = V.  s = |U|.
 *  The cumulant function of U = sum_S g~_n (y_n - mu_n), y_n ~ Bernoulli(mu_n):
 *     K(tau)   = sum_S [log1p(mu_n expm1(g~_n tau)) - tau g~_n mu_n]
 *     K'(tau)  = sum_S mu_n g~_n [1 / ((1 - mu_n) e^(-g~_n tau) + mu_n) - 1]
 *     K''(tau) = sum_S (1 - mu_n) mu_n g~_n^2 e^(g~_n tau) / (1 - mu_n + mu_n e^(g~_n tau))^2
 *     each term in the form that takes only e^(-|g~_n tau|), so neither sign overflows; f64, no fused multiply-add.
 *  Support.  sup = sum_S max(g~_n (1 - mu_n), -g~_n mu_n), inf = sum_S min(the same two).  A tail whose target lies at or beyond its
 *     bound (s >= sup for the upper tail, -s <= inf for the lower) has no saddle point: probability 0, converged, zeta = +-inf.
 *  Root.  For each tail with target c in {+s, -s}, K'(zeta) = c by SPAtest's guarded Newton:
 *         tau = 0, k = K'(tau) - c, prev = +inf
 *         for rep = 1 .. 100:
 *             tau' = tau - k / K''(tau)
 *             tau' not finite: stop, not converged
 *             |tau' - tau| <= 1e-10 (1 + |tau|): zeta = tau', converged
 *             k' = K'(tau') - c
 *             if sign(k) != sign(k'):
 *                 if |tau' - tau| > prev - 1e-10: tau' = tau + sign(k' - k) prev / 2, k' = K'(tau') - c, prev = prev / 2
 *                 else: prev = |tau' - tau|
 *             tau = tau', k = k'
 *  Tail.  w = sign(zeta) sqrt(2 (zeta c - K(zeta))), v = zeta sqrt(K''(zeta)), r = w + log(v / w) / w; the upper tail is 1 - Phi(r),
 *     the lower Phi(r), by gpca_normal_log10p's scheme in log space; the tail fails if r is not finite or has the sign opposite to c.
 *     The two-sided p is the sum of the two tails, formed in log space as max + log1p.
 * spa [rows][T][4] = -log10 p, status, zeta+, zeta- (zeta in the operand's coding: on a flipped row they are those of allele A1 negated
 * and swapped).  status 0: |z| < spa_z or U = 0: the normal value gpca_normal_log10p(z), zeta NaN.  1: the correction applied.  2: a
 * tail did not converge or failed: the normal value (SAIGE's behaviour), zeta what was reached.  Where a13 gives NaN statistics,
 * -log10 p and zeta are NaN and the status is 0.  spa_z is at least 0.5 (below it w and v both tend to 0 and log(v / w) / w cancels) or
 * +inf (no item is corrected); SAIGE's cutoff is 2.
 * Device: the items are flagged and compacted after a13's finish kernel; a workgroup owns an item, reads its row once, keeps g~ in its
 * slice of a workspace bounded independently of the band, and every sum over the samples runs through a fixed tree that depends on N
 * alone (no atomics on sums), so a band is bit-identical to the same rows of the full call and int8, 2-bit and a GPCA_PREC_F32_MFMA
 * handle give the same bits.  GPCA_ASP_SLOTS in the environment, read per call, forces the number of workgroups that walk the item
 * list, clamped to 1 .. the default (at most 1024, fewer once a slice of g~ exceeds 256 KiB); the workspace keeps its size and no
 * result depends on the count: a test hook.  Out of scope: the fast partially-normal variant of SAIGE for non-carriers, and
 * everything a13 leaves out.
 * Errors: those of gpca_assoc_logistic_score, and GPCA_ERR_BAD_ARG for a NULL spa or an spa_z below 0.5 or NaN.
 * gpca_spa_log10p: the same rules for one given vector g~ [n] with mu [n] (in [0, 1]; a sample with mu (1 - mu) = 0 adds nothing) and
 * U = u, sums in sample order; host only, no handle.  Its normal value (u = 0, status 2) is that of u / sqrt(sum mu (1 - mu) g~^2);
 * there is no cutoff: status 0 only for u = 0.  zeta [2] and status may be NULL.  GPCA_ERR_BAD_ARG: a NULL vector or log10p, n < 1, a
 * non-finite g~ or u, a mu outside [0, 1]. */
GPCA_API int gpca_assoc_logistic_spa(gpca_handle* h, const double* Y /* [N][T], 0 / 1 */, int32_t T, const double* C /* [N][Pc] or NULL */,
                                     int32_t Pc, const uint8_t* include /* [N] or NULL */, double max_vif, double spa_z, int64_t row0,
                                     int64_t row1, double* stats /* [rows][T][5] or NULL */, double* spa /* [rows][T][4] */,
                                     double* ua /* [rows][T][Pc + 3] or NULL */, double* rowinfo /* [rows][5] or NULL */);
GPCA_API int gpca_spa_log10p(const double* gt /* [n] */, const double* mu /* [n] */, int64_t n, double u, double* log10p,
                             double* zeta /* [2] or NULL */, int32_t* status /* may be NULL */);

/* ---- a15: the approximate Firth correction of the logistic score scan (Firth 1993; regenie --firth --approx, SAIGE's fallback for the
 * effect size): one coefficient beta on the covariate-adjusted genotype, fitted by the Jeffreys-penalised likelihood with the null
 * model's linear predictor held fixed as an offset.  It is the one correction that also repairs the effect size: for a rare variant
 * whose carriers are all cases a13's beta = U / V means nothing and a maximum-likelihood fit diverges; the Firth estimate is finite.
 * gpca_assoc_logistic_firth is gpca_assoc_logistic_score (the same path: stats, ua and rowinfo carry the same bits) followed by the
 * correction of the items (row, trait) with |z| >= firth_z.
 *  Setting.  That of a14: trait t, kept row i, the operand's coding of a13; g~_n, mu_n, U and Z are those of a14, with the same bits.
 *     eta_n = logit(mu_n) + beta g~_n.  Because X^T W g~ = 0 the unpenalised log-likelihood ratio of that model is
 *     l(beta) - l(0) = beta U - K(beta) with K, K', K'' the functions of a14, its score U - K'(beta), its information K''(beta); y is
 *     not needed on the device.  With Jeffreys' penalty (1/2) log K''(beta):
 *         f(beta) = beta U - K(beta) + (1/2) log(K''(beta) / K''(0))          (f(0) = 0 exactly)
 *         u(beta) = U - K'(beta) + K'''(beta) / (2 K''(beta))
 *         d(beta) = -K''(beta) + (K''''(beta) K''(beta) - K'''(beta)^2) / (2 K''(beta)^2)
 *         K''' = sum_S g~^3 w (1 - 2 p),  K'''' = sum_S g~^4 w (1 - 6 w),  p = mu e^a / (1 - mu + mu e^a), a = g~ beta, w = p (1 - p)
 *     each term, like a14's, in the form that takes only e^(-|a|); f64, no fused multiply-add.  A pass at beta returns
 *     (K, K', K'', K''', K'''').  gmax = max_S |g~_n|.
 *  Root.
 *         beta = 0, P = pass(0), f = 0
 *         for rep = 1 .. 50:
 *             delta = d < 0 ? -u / d : u / K''            (Newton on u; the Fisher step where f is not concave)
 *             delta not finite: stop, failed
 *             |delta| <= 1e-10 (1 + |beta|): converged at beta (the sums in hand are beta's)
 *             |delta| gmax > 5: delta = sign(delta) 5 / gmax
 *             small = |delta| <= 1e-4 (1 + |beta|)
 *             for h = 0 .. 10: beta' = beta + delta 2^-h, P' = pass(beta'), f'; accept if f' is finite, K''(beta') > 0 and (small or f' >= f)
 *             none accepted: stop, failed
 *             beta, P, f = beta', P', f'
 *     50 repetitions without convergence, or K''(0) not positive and finite: failed.  (Without the `small` clause the ascent test
 *     rejects the last Newton steps on rounding alone.)  The answer is the stationary point this rule reaches from 0; u may have more
 *     than one root on a very small sample.
 *  D = max(2 f(beta^), 0); -log10 p = gpca_normal_log10p(sqrt(D)) (chi^2_1); se = 1 / sqrt(K''(beta^)) (logistf's convention); the
 *     reported beta^ is for allele A1: s beta^ with s of a13.
 * firth [rows][T][5] = -log10 p, status, beta^, se, D.  status 0: z is not finite or |z| < firth_z: the normal value
 * gpca_normal_log10p(z), the other three NaN.  1: corrected.  2: the rule failed: the normal value, and beta^, se and D what was
 * reached.  Where a13 gives NaN statistics everything is NaN with status 0.  firth_z >= 0, or +inf (no item is corrected, and no input
 * of the correction is built or allocated); 1.959964 is the two-sided 0.05 of regenie's --pThresh.
 * Device: a14's, with a kernel of its own (assoc_firth.hip): the same flagging and compaction, item ranges, workspace and fixed
 * summation tree, so a band is bit-identical to the same rows of the full call and int8, 2-bit and a GPCA_PREC_F32_MFMA handle give
 * the same bits; GPCA_ASP_SLOTS (a14: a test hook, read per call) forces this kernel's workgroup count too, and no result depends on
 * it.  Out of scope: the exact Firth test with the covariates refitted per SNP, a Firth-penalised null fit,
 * profile-likelihood intervals, regenie's own numbers (its choices of offset and of genotype coding are not claimed), and everything
 * a13 leaves out (streamed and row-sharded handles: GPCA_ERR_STATE).
 * Errors: those of gpca_assoc_logistic_score, and GPCA_ERR_BAD_ARG for a NULL firth or a firth_z that is negative or NaN.
 * gpca_firth_log10p: the same rules for one given vector g~ [n] with mu [n] (in [0, 1]; a sample with mu (1 - mu) = 0 adds nothing)
 * and U = u, sums in sample order; host only, no handle; out [5] as above with beta^ in the given coding.  There is no cutoff: status
 * is 1 or 2, and the normal value of status 2 is that of u / sqrt(sum mu (1 - mu) g~^2).  GPCA_ERR_BAD_ARG: a NULL vector or out,
 * n < 1, a non-finite g~ or u, a mu outside [0, 1]. */
GPCA_API int gpca_assoc_logistic_firth(gpca_handle* h, const double* Y /* [N][T], 0 / 1 */, int32_t T, const double* C /* [N][Pc] or NULL */,
                                       int32_t Pc, const uint8_t* include /* [N] or NULL */, double max_vif, double firth_z, int64_t row0,
                                       int64_t row1, double* stats /* [rows][T][5] or NULL */, double* firth /* [rows][T][5] */,
                                       double* ua /* [rows][T][Pc + 3] or NULL */, double* rowinfo /* [rows][5] or NULL */);
GPCA_API int gpca_firth_log10p(const double* gt /* [n] */, const double* mu /* [n] */, int64_t n, double u, double* out /* [5] */);

/* ---- a16: gene-level set tests of the logistic score scan (regenie --vc-tests, SAIGE-GENE, SKAT): the rare variants of one gene tested
 * together.  gpca_assoc_logistic_set is gpca_assoc_logistic_score over the LISTED rows of n_sets sets (stats, ua and rowinfo of a listed
 * row carry the bits gpca_assoc_logistic_score gives that row), followed by the covariance of the scores inside every set,
 * Phi = G~^T W G~ per trait; gpca_set_test turns the scores and Phi of one set into a burden and a SKAT p-value on the host.
 *  Setting.  That of a13 / a14: trait t, the included samples S, w = mu (1 - mu) as the f32 panel column a13 multiplies; a kept row i
 *     has the exact integers n_obs, s1, s2 and its flip; its operand x (g, or 2 - g on a flipped row, where observed and in S, else
 *     0), m = [missing and in S], xbar the operand's mean, a_i,j (j = 0 .. Pc) the values ua reports.  x~ = x + xbar m and
 *     g~_i = x~_i - sum_j a_i,j Z_j, so that g~_i^T W g~_i = V_i.
 *  Per pair (a, b), b <= a, of rows of one set and per trait, four sums over the samples:
 *         XX = sum x_a x_b w,   XM = sum x_a m_b w,   MX = sum m_a x_b w,   MM = sum m_a m_b w
 *     with f32 operands x_a or m_a on one side and w x_b or w m_b (w, 2 w or 0: exact) on the other, every product exact.  The
 *     accumulation is a13's: the 16-sample group order (i, 8 + i); an f32 accumulator holds at most 256 samples, counted from sample 0,
 *     before it is added to an f64 running sum; no split of the sample axis, no atomics; the M sums run only in groups where a wave
 *     ballot finds a missing call (a product of 0 more or less changes no sum).  Then in f64, no fused multiply-add, in this order:
 *         R_ab       = (XX + (xbar_b XM + xbar_a MX)) + (xbar_a xbar_b) MM
 *         q_ab       = sum_{j = 1 .. Pc} a_a,j a_b,j           (from 0, j ascending)
 *         Phi^op_ab  = (R_ab - a_a,0 a_b,0) - q_ab
 *         Phi_ab     = s_a s_b Phi^op_ab,   s = -1 on a flipped row (allele A1's coding: the projection annihilates the constant the
 *                      flip adds)
 *     On the diagonal XM = MX = 0 and MM = e[w]: R_aa is a13's gwg and Phi_aa carries the bits of a13's V.  An entry with a row of
 *     n_obs = 0 is NaN.
 *  The call.  set_off [n_sets + 1] (set_off[0] = 0) cuts set_rows into the sets; each lists 1 <= m <= GPCA_SET_MAX_ROWS rows, strictly
 *     ascending, in [0, K) in PCA-SNP order; a row may appear in several sets (it is then listed, and computed, once per set).
 *     stats [listed][T][5], ua [listed][T][Pc + 3], rowinfo [listed][5] as in a13, each may be NULL; phi (required): set after set,
 *     per set trait after trait, per trait the packed lower triangle of m (m + 1) / 2 entries row by row ((a, b) at a (a + 1) / 2 + b).
 *     A Phi entry depends on its two rows, S, N and the trait alone: not on the set's other rows, the pair's position, the other
 *     sets of the call or the storage mode (int8, 2-bit, a GPCA_PREC_F32_MFMA handle).
 *     Errors: a13's, and GPCA_ERR_BAD_ARG for a NULL phi, n_sets < 1, a set that is empty, longer than GPCA_SET_MAX_ROWS or not strictly
 *     ascending (gpca_last_error names the set's index) and a row outside [0, K); GPCA_ERR_OOM is checked before any allocation;
 *     streamed and row-sharded handles: GPCA_ERR_STATE.
 *  gpca_set_test (host only, no handle; f64, no fused multiply-add): u [m] = the scores for allele A1 (s U), phi = the packed lower
 *     triangle, weight [m] or NULL = 1 (a NaN or negative weight, m < 1 or m > GPCA_SET_MAX_ROWS, a NULL u, phi or out: GPCA_ERR_BAD_ARG).
 *     Rows used: u finite, Phi_ii finite and > 0, weight finite and > 0; with omega their weights and A_ij = (omega_i Phi_ij) omega_j:
 *     out [10] = m_used, burden beta, burden se, burden z, burden -log10 p, SKAT Q, SKAT -log10 p, SKAT status, z_Q, zeta; with
 *     m_used = 0 everything after it is NaN and the status 0.
 *     Burden.  t_i = omega_i u_i; B = sum t_i; v = sum_i sum_j A_ij (i, then j, ascending); z = B / sqrt(v), beta = B / v,
 *         se = 1 / sqrt(v), -log10 p = gpca_normal_log10p(z); all NaN unless v > 0.
 *     SKAT.  Q = sum t_i^2.  lambda = the eigenvalues of A, descending, from the function behind gpca_host_eigh_desc; those above
 *         (mean of the non-negative lambda) / 1e5 are kept (the SKAT package's rule; none kept, or an A that is not finite: Q alone
 *         is reported).  c1 = sum lambda, c2 = sum lambda^2, z_Q = (Q - c1) / sqrt(2 c2).
 *         bulk = -log10(1 - Phi_N(x)) with kappa = c2 / c1, nu = c1 c1 / c2, h = 2 / (9 nu),
 *                x = (cbrt(Q / (kappa nu)) - (1 - h)) / sqrt(h)            (Satterthwaite, Wilson-Hilferty)
 *             the one-sided normal tail in log space: gpca_normal_log10p(x) + log10(2) for x >= 0, -log1p(-erfc(-x / sqrt 2) / 2) / ln 10
 *             below.
 *         status 0 (z_Q < 0.5 or NaN; a14's cutoff for a14's reason: w and v of the tail both tend to 0 there): bulk, zeta NaN.
 *         otherwise Kuonen's saddle point with K(zeta) = -(1/2) sum log1p(-2 zeta lambda), K' = sum lambda / (1 - 2 zeta lambda),
 *         K'' = 2 sum (lambda / (1 - 2 zeta lambda))^2.  The root of K' = Q on (lo, hi) = (0, ub), ub = 1 / (2 lambda_1):
 *             zeta = (Q - c1) / (2 c2); outside (lo, hi): zeta = (lo + hi) / 2
 *             for rep = 1 .. 200:
 *                 f = K'(zeta) - Q;  f not finite: stop, no root
 *                 f > 0: hi = zeta, else lo = zeta
 *                 zeta' = zeta - f / K''(zeta);  outside (lo, hi): zeta' = (lo + hi) / 2
 *                 found = |zeta' - zeta| <= 1e-10 ub;  zeta = zeta';  stop when found
 *         w = sqrt(2 (zeta Q - K)), v = zeta sqrt(K''), r = w + log(v / w) / w at the final zeta.
 *         status 1: a root was found and r is finite and > 0: -log10 p = the one-sided tail of r.
 *         status 2: otherwise: bulk (zeta = what was reached).
 *  Not there: SKAT-O and ACAT; collapsing of ultra-rare variants and sets above GPCA_SET_MAX_ROWS; quantitative traits; SAIGE-GENE+'s
 *     rescaling of Phi from saddle-point p-values (the set tests inherit the normal approximation at extreme case imbalance); Davies'
 *     method; annotation and mask files; streamed and row-sharded handles. */
#define GPCA_SET_MAX_ROWS 128
GPCA_API int gpca_assoc_logistic_set(gpca_handle* h, const double* Y /* [N][T], 0 / 1 */, int32_t T, const double* C /* [N][Pc] or NULL */,
                                     int32_t Pc, const uint8_t* include /* [N] or NULL */, double max_vif, int32_t n_sets,
                                     const int64_t* set_off /* [n_sets + 1] */, const int64_t* set_rows /* [set_off[n_sets]] */,
                                     double* stats /* [listed][T][5] or NULL */, double* ua /* [listed][T][Pc + 3] or NULL */,
                                     double* rowinfo /* [listed][5] or NULL */, double* phi /* per set [T][m (m + 1) / 2] */);
GPCA_API int gpca_set_test(const double* u /* [m] */, const double* phi /* [m (m + 1) / 2] */, const double* weight /* [m] or NULL */,
                           int32_t m, double* out /* [10] */);

/* ---- a17: genotype counts inside sample groups, and Fst from them (plink --freq --within / --fst, smartpca's Fst table): what a SNP
 * looks like inside each of P groups of samples -- populations, or cases and controls.
 * gpca_group_counts: group [N] labels every sample with its group 0 .. P - 1 or with -1 (any negative label: in no group); a group
 *     without a sample is allowed.  For the kept rows [row0, row1) in PCA-SNP order, counts [rows][P][3] (uint32) = n_obs, n_het, n_hom2:
 *     the samples of the group with an observed call on the row, those with g = 1 and those with g = 2 (g counts copies of A1).
 *  Device: 0/1 indicator bytes of the calls ([g = 1], [g = 2], [missing]) times the 0/1 one-hot matrix of the labels on
 *     v_mfma_i32_32x32x32_i8, in i32: exact integers, n_obs = the group's size - its missing calls; the missing plane runs only in
 *     blocks of 32 samples where a wave ballot over 32 rows finds a missing call (a product of 0 more or less changes no sum); 33 .. 64
 *     groups read the genotypes once; no split of the sample axis, no atomics, every count written once.  A sample at or beyond N and
 *     a sample with label -1 have an all-zero one-hot column.
 *     A band is bit-identical to the same rows of the full call; int8 and 2-bit residency and a GPCA_PREC_F32_MFMA handle give the
 *     same counts; the sample mask is ignored and no fitted result is touched.
 *  Errors: GPCA_ERR_STATE (no standardisation, K = 0, a streamed handle, a row-sharded handle), GPCA_ERR_BAD_ARG (a NULL group or
 *     counts, P outside 1 .. GPCA_GROUPS_MAX, a label >= P, a row range out of bounds), GPCA_ERR_INVALID_GENOTYPE (a row the call
 *     reads holds a value outside {0, 1, 2, missing} on a sample below N, in a group or not; the message names the row, as in a12),
 *     GPCA_ERR_OOM (checked before any allocation).
 * The two Fst rules are host only, take no handle, work in f64 with no fused multiply-add and read counts [rows][P][3].  Per group
 * i of a row: n_i = 2 n_obs (allele count, formed in f64), p_i = (n_het + 2 n_hom2) / n_i.  Both add row by row, rows ascending, to the
 * caller's running sums (zero them before the first band): calls over consecutive bands give the bits of one call over all rows.
 *  gpca_fst_hudson (Hudson's estimator as in Bhatia et al. 2013; plink 2's default): per pair (i, j), j < i, at pair index
 *     i (i - 1) / 2 + j of P (P - 1) / 2, per row:
 *         d   = p_i - p_j
 *         num = (d d - (p_i (1 - p_i)) / (n_i - 1)) - (p_j (1 - p_j)) / (n_j - 1)
 *         den = p_i (1 - p_j) + p_j (1 - p_i)
 *     A row contributes to the pair iff both groups have n_obs >= 1; otherwise num and den are NaN and nothing is added.
 *     sums [pairs][3] += num, den, 1 (pairs ascending inside a row); the genome-wide value is sums[.][0] / sums[.][1].  num and den
 *     [rows][pairs] may each be NULL.  GPCA_ERR_BAD_ARG: NULL counts or sums, rows < 0, P outside 2 .. GPCA_GROUPS_MAX.
 *  gpca_fst_wc (Weir and Cockerham 1984) over the groups with use[p] != 0 (NULL: all), r of them, ascending; n_i = n_obs here,
 *     h_i = n_het / n_i, p_i as above; every sum from 0, groups ascending:
 *         n_t = sum n_i,  q = sum n_i n_i
 *         nbar = n_t / r,  n_c = (n_t - q / n_t) / (r - 1),  pbar = (sum n_i p_i) / n_t,  hbar = (sum n_i h_i) / n_t
 *         s2 = (sum n_i ((p_i - pbar) (p_i - pbar))) / ((r - 1) nbar)
 *         core = pbar (1 - pbar) - ((r - 1) / r) s2
 *         a = (nbar / n_c) (s2 - (core - hbar / 4) / (nbar - 1))
 *         b = (nbar / (nbar - 1)) (core - ((2 nbar - 1) / (4 nbar)) hbar)
 *         c = hbar / 2
 *     A row contributes iff every used group has n_obs >= 1 and n_t > r; otherwise a, b, c are NaN and nothing is added.
 *     sums [3] += a, (a + b) + c, 1; the genome-wide value is sums[0] / sums[1].  abc [rows][3] may be NULL.  GPCA_ERR_BAD_ARG: NULL
 *     counts or sums, rows < 0, P outside 1 .. GPCA_GROUPS_MAX, fewer than two groups used.
 *  Not there: per-variant dropping of samples, haploid and sex chromosomes, weighted or hierarchical F-statistics, jackknife standard
 *     errors, more than GPCA_GROUPS_MAX groups, streamed and row-sharded handles. */
#define GPCA_GROUPS_MAX 64
GPCA_API int gpca_group_counts(gpca_handle* h, const int32_t* group /* [N] */, int32_t P, int64_t row0, int64_t row1,
                               uint32_t* counts /* [rows][P][3] */);
GPCA_API int gpca_fst_hudson(const uint32_t* counts, int64_t rows, int32_t P, double* num /* [rows][pairs] or NULL */,
                             double* den /* same or NULL */, double* sums /* [pairs][3]: sum num, sum den, rows used; ADDED TO */);
GPCA_API int gpca_fst_wc(const uint32_t* counts, int64_t rows, int32_t P, const uint8_t* use /* [P] or NULL */,
                         double* abc /* [rows][3] or NULL */, double* sums /* [3]: sum a, sum (a + b + c), rows used; ADDED TO */);

/* ---- a18: genotype counts per sample, and the heterozygosity F from them (plink --missing's sample table and --mind, plink --het):
 * what a sample looks like over the SNPs.  Contamination gives a strongly negative F, inbreeding or a failed array a positive one.
 * gpca_sample_counts: for the kept rows [row0, row1) in PCA-SNP order, counts [N][3] (uint32) = n_obs, n_het, n_hom2 of every sample:
 *     the band's rows on which it has an observed call, those with g = 1 and those with g = 2 (g counts copies of A1).  With q
 *     [row1 - row0] (each at most 2^30) qsum [N] (uint64) = the sum of q[j] over the band's rows j on which the sample is observed; q and
 *     qsum are both given or both NULL.  The outputs are WRITTEN, not added to (an empty band writes zeros): the caller sums its bands.
 *  Device: a reduction over the SNP axis.  A thread owns 16 consecutive samples (one 16-byte load of an int8 row, one dword of a 2-bit
 *     row); the missing, het and hom2 indicators are added byte-wise (four counters to a dword) and the bytes are added to 32-bit
 *     registers once per 248 rows, before one can wrap; qsum = (the sum of all q of the band) - (the q of the sample's missing calls) in
 *     64-bit integers, the per-sample work only on rows where a wave ballot finds a missing call.  The band's rows are split over
 *     workgroups; each split writes its sums once and a second kernel adds them: integers, so the split changes no bit
 *     (GPCA_SAMPLE_COUNTS_SPLITS in the environment, read per call, forces the split count, clamped to 1 .. rows: a test hook).  No
 *     float touches a sum.  A sample at or beyond N never contributes, whatever the pad bytes hold.
 *     A call over all rows equals the sum of calls over consecutive bands; int8 and 2-bit residency and a GPCA_PREC_F32_MFMA handle give
 *     the same bits; the sample mask is ignored and no fitted result is touched.
 *  Errors: GPCA_ERR_STATE (no genotypes, a streamed handle, a row-sharded handle, no standardisation, K = 0), GPCA_ERR_BAD_ARG (a NULL
 *     counts, q without qsum or the reverse, a q[j] above 2^30, a row range out of bounds, a band of 2^31 or more rows),
 *     GPCA_ERR_INVALID_GENOTYPE (a row the call reads holds a value outside {0, 1, 2, missing} on a sample below N; the message names
 *     the row, as in a12), GPCA_ERR_OOM (checked before any allocation).
 * The two host rules take no handle and work in f64 with no fused multiply-add, in exactly this order.
 *  gpca_het_weights: qc [rows][4] = n_valid, n_hom0, n_het, n_hom2 as gpca_get_snp_qc_detail gives them.  Per row, every count formed
 *     in f64:
 *         t = 2 n_valid,  p = (n_het + 2 n_hom2) / t
 *         e = ((2 p) (1 - p)) (t / (t - 1))          the unbiased expected heterozygosity of the row (plink 1.9's small-sample term)
 *         q = (uint32) floor(e 2^30 + 0.5)
 *     A row with n_valid = 0 gets q = 0.  e <= 1 (2 p (1 - p) <= 1/2, t / (t - 1) <= 2), so q <= 2^30.
 *     GPCA_ERR_BAD_ARG: NULL qc or q, rows < 0.
 *  gpca_sample_het: counts [N][3] and qsum [N] as gpca_sample_counts gives them (summed over the bands), with q from gpca_het_weights.
 *     Per sample, n_obs, n_het and qsum converted to f64 (qsum rounds to nearest above 2^53):
 *         O_HOM = n_obs - n_het,  E_HOM = n_obs - qsum / 2^30,  d = n_obs - E_HOM,  F = (O_HOM - E_HOM) / d
 *     out [N][3] = O_HOM, E_HOM, F; F is NaN where n_obs = 0 or d <= 0.  GPCA_ERR_BAD_ARG: a NULL argument, N < 0.
 *  plink's own printed digits are not claimed: plink 1.9 takes the allele frequencies of --het from the loaded samples too, but rounds
 *     in its own order.
 *  Not there: haploid and sex chromosomes and a sex check, an iterated heterozygosity filter, per-sample weights other than one u32 per
 *     row, streamed and row-sharded handles. */
GPCA_API int gpca_sample_counts(gpca_handle* h, int64_t row0, int64_t row1, const uint32_t* q /* [row1 - row0] or NULL */,
                                uint32_t* counts /* [N][3] */, uint64_t* qsum /* [N] or NULL */);
GPCA_API int gpca_het_weights(const uint32_t* qc /* [rows][4] */, int64_t rows, uint32_t* q /* [rows] */);
GPCA_API int gpca_sample_het(const uint32_t* counts /* [N][3] */, const uint64_t* qsum /* [N] */, int64_t N, double* out /* [N][3] */);

/* ---- a19: LD scores from the windowed-LD sweep, and LD-score regression (Bulik-Sullivan et al. 2015) on a scan's statistics: does the
 * inflation of the test statistics come from confounding (the intercept) or from polygenic signal (the slope = SNP heritability)?
 * gpca_ld_score: the sweep of a10 over the same band, with the same addressing, the same win_end contract and the same checks; the
 *     six pair counts never leave the device.  For every pair (i, j) of the band's windows, from the counts and in f64 as in a10,
 *         cov = n sxy - sx sy,  vx = n sxx - sx sx,  vy = n syy - sy sy,  r2 = (cov cov) / (vx vy)      (the bits of a10's r2)
 *     A pair with vx <= 0, vy <= 0 or n <= 2 is SKIPPED: it adds to nothing and is not counted.  A counted pair is worth
 *         v = r2 - (1.0 - r2) / (n - 2.0)   with GPCA_LDSCORE_UNBIASED (ldsc's bias adjustment, with the pair's own jointly observed n)
 *         v = r2                            without
 *         q = (int64) rint(v 2^40), half to even; no fused multiply-add in this chain
 *     and q is added to score[i - row0] AND to score[j - row0], 1 to partners[...] at the same two places.  The unit of score is 2^-40.
 *     score and partners hold span = min(K, row1 + wmax) - row0 entries from row0 and are WRITTEN (zeros where no pair reaches).
 *     Every sum is an integer, so tiling, order and atomics move no bit: the sum over consecutive bands, each added at its row0, is the
 *     full call (the caller adds its bands; a SNP's LD score needs the windows of the rows before it too), and int8 and 2-bit residency
 *     and a GPCA_PREC_F32_MFMA handle give the same bits.  rows = 0 returns GPCA_OK and writes nothing.  The sample mask is ignored
 *     (every sample enters) and no fitted result of the handle is touched.  wmax <= 2^20, so that 2 wmax pairs of at most 2^41 stay
 *     below 2^63.
 *  Device: one kernel after the sweep reads the six i32 planes once (24 B per slot).  A workgroup takes 64 rows x 256 slots; thread p
 *     owns partner row t0 + d0 + 1 + p and walks the tile's rows, so each step reads consecutive slots of one row and the partner's sum
 *     stays in registers; the row's own sum is a wave reduction and one LDS atomic per wave; one 64-bit and one 32-bit global atomic per
 *     touched row and tile.
 *  Errors: GPCA_ERR_STATE (no genotypes, a streamed handle, a row-sharded handle, no standardisation, K = 0), GPCA_ERR_BAD_ARG (ranges,
 *     win_end, wmax < 1, wmax > 2^20, a NULL score, unknown flag bits, 4 N >= 2^31), GPCA_ERR_INVALID_GENOTYPE (a row the call reads
 *     holds a value outside {0, 1, 2, missing}; the message names the row), GPCA_ERR_OOM (checked before any allocation).
 * The two host rules take no handle and work in f64 with no fused multiply-add.
 *  gpca_ld_score_total: l2[i] = 1 + acc[i] 2^-40 (acc = the bands' scores added up; the 1 is the SNP with itself).
 *  gpca_ldsc_fit: chi2, ell, w_ell [m] (w_ell NULL = ell); N = n_samples, M = the number of SNPs the LD scores sum over.
 *   1. Used rows: those with finite chi2, ell, w_ell and, when chi2_max > 0, chi2 <= chi2_max, in the given order; m_used of them.
 *      B = min(n_blocks, m_used).  GPCA_ERR_BAD_ARG when B < 2, m_used < 3, n_samples <= 0 or M <= 0.
 *   2. Start: h = clamp(M (mean chi2 - 1) / (N mean l'), 0, 1), a = 1, with l' = max(ell, 1) and wl' = max(w_ell, 1).
 *   3. Weights: w_j = 1 / (wl'_j 2 (a + N clamp(h, 0, 1) l'_j / M)^2)   (ldsc's heteroskedasticity and over-counting weights).
 *   4. Solve: weighted least squares of chi2 on (1, l').  The five sums sum w, sum w l, sum w l^2, sum w chi2, sum w l chi2 are
 *      accumulated sequentially in f64 per jackknife block (block k = used rows [floor(m_used k / B), floor(m_used (k + 1) / B))); the
 *      totals are the block sums added in block order; the 2 x 2 system is solved by its determinant, and a determinant <= 0 or
 *      non-finite is GPCA_ERR_BAD_ARG (constant ell).  That gives the intercept a and the slope b; h = b M / N.
 *   5. Reweighting: two rounds of (solve, recompute the weights from (a, h)), then a final solve: three solves.
 *   6. Delete-one jackknife over the B blocks with the final weights: estimates from totals minus block sums, pseudo-values
 *      B theta - (B - 1) theta_(k), se = sqrt(var(pseudo, ddof = 1) / B).
 *   7. out [10] = m_used, mean chi2, lambda_GC = median chi2 / 0.4549364231195724 (an even count: the mean of the middle two),
 *      intercept, its se, h2, its se, ratio = (a - 1) / (mean chi2 - 1) and its se = se_a / (mean chi2 - 1) (both NaN when
 *      mean chi2 <= 1), B.
 *   h2 of a binary trait is on the observed scale.  ldsc's two-step estimator and its printed digits are not claimed.
 *  Not there: LD clumping of scan results, partitioned or annotation-stratified LD scores, cM windows (there is no genetic map), ldsc's
 *     two-step estimator, genetic correlation, liability-scale conversion, streamed and row-sharded handles. */
#define GPCA_LDSCORE_UNBIASED 1
GPCA_API int gpca_ld_score(gpca_handle* h, int64_t row0, int64_t row1, const int64_t* win_end /* [row1 - row0] */, int32_t wmax,
                           int32_t flags, int64_t* score /* [span], units of 2^-40 */, int32_t* partners /* [span]; may be NULL */);
GPCA_API int gpca_ld_score_total(const int64_t* acc /* [K] */, int64_t K, double* l2 /* [K] */);
GPCA_API int gpca_ldsc_fit(const double* chi2, const double* ell, const double* w_ell /* NULL = ell */, int64_t m, double n_samples, double M,
                           int32_t n_blocks, double chi2_max, double* out /* [10] */);

/* ---- a20: runs of homozygosity (plink --homozyg): per sample, the stretches of consecutive kept SNPs that a sliding window calls
 * homozygous, and from them F_ROH, the share of the genome inside runs.  Where a18's F is one number per sample, the runs tell a sample
 * with a few long autozygous tracts (recent consanguinity) from one whose excess homozygosity is spread thin.
 * gpca_roh works on the kept rows [row0, row1) of a resident handle, in PCA-SNP order, and on all N samples (the sample mask is
 * ignored, as in a18).  A call is 0, 1, 2 or missing; "het" means 1.
 *  brk [row1 - row0], one byte per row: bit 0 = a window domain starts at this row (a new chromosome); bit 1 = a run may not continue
 *     from the previous row into this one (a new chromosome, or a gap above the caller's limit).  Bit 0 without bit 1, or any other bit
 *     set, is GPCA_ERR_BAD_ARG naming the row.  Row row0 is taken as 3 whatever it holds: a band is a world of its own, and the caller
 *     cuts its bands at domain starts.
 *  gpca_roh_params: window_snp W (1 .. GPCA_ROH_WINDOW_MAX = 64); window_het H and window_missing M (each 0 .. W); thr_num and thr_den
 *     (0 <= num <= den, 1 <= den <= 2^20); min_snp >= 1; max_het (-1 = no limit, else >= 0).
 *  1. Windows.  Inside a domain of L rows, window s covers rows s .. s + W - 1 of the domain, s = 0 .. L - W; a domain shorter than W has
 *     no window.  For a sample, window s is a hit iff its het calls <= H and its missing calls <= M.
 *  2. SNPs.  Row j of the domain is covered by the windows s with max(0, j - W + 1) <= s <= min(j, L - W); cov = their number, hits = the
 *     number of them that are hits for the sample.  The row is in-ROH for the sample iff cov > 0 and hits den >= num cov: exact
 *     integers, no float decides a row.
 *  3. Runs.  A run is a maximal stretch of consecutive kept rows that are in-ROH for the sample, cut before every row with bit 1 set.
 *     Its record is five uint32: (sample, first, last, n_het, n_missing); first and last are kept-row indices of the handle (absolute,
 *     not relative to the band), n_het and n_missing the sample's het and missing calls on the run's rows.  A run is reported iff
 *     last - first + 1 >= min_snp and (max_het < 0 or n_het <= max_het).
 *  4. Output.  seg_count [N] (uint32) = the reported runs of every sample, always complete; *n_found = their sum; segs [cap][5] = the
 *     first min(cap, n_found) records in ascending (sample, first) order.  n_found > cap is GPCA_OK: the caller comes back with a larger
 *     buffer.  segs may be NULL iff cap = 0.  An empty band writes zeros.  The order and every value are independent of the launch
 *     plan; int8 and 2-bit residency and a GPCA_PREC_F32_MFMA handle give the same bits; no fitted result is touched.
 *  Device: the access pattern of a18 (a thread owns 16 consecutive samples, a workgroup 1 024 samples and one row split).  A first
 *     kernel keeps, per sample, byte-wise running het and missing counts of the last W rows (the entering row added, the row W behind
 *     fetched again and subtracted) and the hits among the last W windows (a window's hit bits wait in a ring of 64 windows in LDS
 *     until they leave), decides row j when the last window that covers it completes (W - 1 rows later, or at the domain's end), and
 *     writes one bit per (row, sample); a split reads a halo of W - 1 rows on either side, clipped at the domain.  A second kernel, run
 *     as a count pass and as a fill pass, walks the bits over its split's rows, fetching genotypes only where a wave ballot finds a
 *     run; what crosses a boundary between two splits is joined by a third kernel, a thread per sample; an exclusive scan of the
 *     counts (per sample over the splits on the device, over the samples on the host) puts the fill in order.  No float, no atomic
 *     on an output.  GPCA_ROH_SPLITS in the environment, read per call, forces the split count, clamped to 1 .. rows: a test hook.
 *  Errors: GPCA_ERR_STATE (no genotypes, a streamed handle, a row-sharded handle, no standardisation, K = 0), GPCA_ERR_BAD_ARG (a NULL
 *     brk, params, seg_count or n_found; segs NULL with cap > 0; cap < 0; a row range out of bounds; a band of 2^31 or more rows; K of
 *     2^32 or more; a bad brk byte; a parameter out of range), GPCA_ERR_INVALID_GENOTYPE (a row of the band holds a value outside
 *     {0, 1, 2, missing} on a sample below N; the message names the row, as in a12), GPCA_ERR_OOM (checked before any allocation).
 * Length in bp and SNP density need positions; they are a host rule on the records, in integers.
 *  gpca_roh_select: segs [n][5] as gpca_roh gives them, pos [K] = the position of every kept row.  span = pos[last] - pos[first];
 *     keep[i] = 1 iff span >= min_bp and span <= max_bp_per_snp (last - first + 1), else 0.  GPCA_ERR_BAD_ARG: a NULL argument with n > 0,
 *     n < 0, min_bp < 0, max_bp_per_snp < 0, a record with last < first.
 *  Not there: W > 64; plink's own printed digits and its float comparison at the threshold; overlap pools and consensus segments
 *     (--homozyg-group); kb-based scanning windows; haploid and sex chromosomes; streamed and row-sharded handles. */
#define GPCA_ROH_WINDOW_MAX 64
typedef struct gpca_roh_params {
    int32_t window_snp, window_het, window_missing;
    int32_t thr_num, thr_den;
    int32_t min_snp, max_het;
} gpca_roh_params;
GPCA_API int gpca_roh(gpca_handle* h, int64_t row0, int64_t row1, const uint8_t* brk /* [row1 - row0] */, const gpca_roh_params* params,
                      uint32_t* seg_count /* [N] */, uint32_t* segs /* [cap][5]; NULL iff cap = 0 */, int64_t cap, int64_t* n_found);
GPCA_API int gpca_roh_select(const uint32_t* segs /* [n][5] */, int64_t n, const int64_t* pos /* [K] */, int64_t min_bp,
                             int64_t max_bp_per_snp, uint8_t* keep /* [n] */);

/* ---- a21: admixture proportions (the ADMIXTURE model, fitted by EM with SQUAREM acceleration): how much of every sample comes from each
 * of K ancestral populations, and the A1 frequency of every kept SNP in each of them.  The calls work on ALL kept rows of a resident
 * handle under its current keep mask, in PCA-SNP order (Kr = gpca_num_pca_snps rows), and on all N samples; the sample mask is ignored
 * and `mode` alone says what a sample does.  A call is 0, 1, 2 (copies of A1) or missing; a missing call contributes nothing anywhere.
 *  Q [N][K] f32, rows on the simplex; F [Kr][K] f32, the A1 frequency of each ancestry; 1 <= K <= GPCA_ADMIX_MAX_K = 16;
 *  eps = (float)1e-5, hi = (float)1 - eps (f32 subtraction).
 *  mode [N] uint8 or NULL (all 0): 0 = Q free, the sample contributes to F; 1 = Q stays as given, the sample contributes to F (a
 *     reference sample of known ancestry); 2 = Q free, the sample does not contribute to F (a projected sample: a relative, a QC failure).
 *  One EM step (Q, F) -> (Q', F', loglik), every quantity a sum, product or quotient of non-negative f32 numbers:
 *   p1 = sum_k q_jk f_ik and p0 = sum_k q_jk (1 - f_ik) (k ascending, fused multiply-adds; p0 is its own dot product, never 1 - p1);
 *   a = g / p1 and b = (2 - g) / p0 for an observed call, both 0 for a missing one;
 *   loglik = the sum over observed calls of g log p1 + (2 - g) log p0: log is the device library's f32 logf, the terms (with g = 0 and
 *     2 - g = 0 terms left out) are added in f64, and all samples enter whatever their mode;
 *   F side, over the samples with mode != 2: AQ_ik = sum_j a q_jk, BQ_ik = sum_j b q_jk; num = f_ik AQ_ik, den = num + (1 - f_ik) BQ_ik;
 *     f'_ik = min(max(num / den, eps), hi); a row with den = 0 (no observed call among the contributors) keeps f;
 *   Q side, over the kept rows: S_jk = sum_i (a f_ik, then b (1 - f_ik)); t_jk = q_jk S_jk; x_k = max(t_jk / sum_k t_jk, eps);
 *     q'_jk = x_k / sum_k x_k; a sample with no observed call (sum_k t_jk = 0) or with mode 1 keeps its row.
 *  Summation shape: no float atomics; the order of every sum is a function of (Kr, N, K) alone -- never of the CU count, the
 *     environment, the storage mode or the handle's precision.  Samples are cut into chunks of 256, kept rows into blocks of 4 096
 *     (plan_math.h, adm_plan).  A sum over samples (AQ, BQ) is formed inside a chunk as 16 groups of 16 consecutive samples, each group
 *     ascending, the groups added ascending; the chunks' sums go to a slab and are added ascending.  A sum over rows (S) is formed
 *     row by row ascending inside a block; the blocks' sums go to a slab and are added ascending.  loglik: per sample over the block's
 *     rows ascending, then the chunk's 256 samples ascending, then the (block, chunk) partials p = block * chunks + chunk: stride-256
 *     classes (p, p + 256, ...) ascending each, then the 256 class sums ascending.  So int8 and 2-bit residency, a GPCA_PREC_F32_MFMA
 *     handle and any two calls with the same inputs give the same bits.
 *  gpca_admix_init: a pure function of (seed, K, N, Kr, the kept rows' observed A1 frequencies).  u(stream, index, k) = ((w >> 9) + 0.5)
 *     2^-23 with w = word k & 3 of philox4x32-10(counter = (index low word, index high word, k >> 2, stream), key = (seed low word, seed
 *     high word)).  Q, stream 0x41444D51, index = the sample: x_k = 0.1f + 0.9f u (f32, product then sum), q_jk = x_k / sum_k x_k (k
 *     ascending).  F, stream 0x41444D46, index = the kept row (0 .. Kr - 1): freq_i = (float)((n_het + 2 n_hom2) / (2 n_valid)) of the
 *     row's counts as gpca_get_snp_qc_detail gives them (the division in f64; 0.5 where n_valid = 0), f_ik = min(max(freq_i (0.5f + u),
 *     eps), hi) in f32.  The counts are those of the resident genotypes whenever the call is accepted: an upload drops the statistics,
 *     and gpca_set_standardization on a handle without them runs the counting pass of gpca_snp_stats (no filter) first, so they count
 *     every sample's calls whichever of the two prepared the handle.
 *  gpca_admix_step: the step above on the caller's Q and F exactly as given (a Q row must be non-negative with a positive sum, an F
 *     value in [0, 1]; every function here leaves F in [eps, hi] and Q positive, and a caller who passes zeros gets IEEE's infinities).
 *     The building block of the fit, and its test hook.
 *  gpca_admix: the fit.  params: K, seed, max_iter (counts steps), tol (relative), accel (0 or 1), init (0 = gpca_admix_init(seed); 1 =
 *     the caller's Q and F, clamped: F to [eps, hi], and a row of Q with mode != 1 that holds a value below eps to max(q, eps) / their
 *     sum).  While steps < max_iter, a cycle from theta0:
 *      1. step theta0 -> theta1, l0; trace[cycle] = l0 (while it fits the capacity);
 *      2. stop, converged, when a cycle before this one exists and l0 - l0_prev < tol |l0|: the result is theta1;
 *      3. accel = 0, or max_iter reached: continue from theta1;
 *      4. accel = 1 (SQUAREM S3): step theta1 -> theta2, l1; r = theta1 - theta0, v = theta2 - theta1 - r, per element in f64; the sums of
 *         r^2 and of v^2 run over Q then F, in blocks of 4 096 elements (stride-256 classes ascending, the 256 class sums ascending), the
 *         blocks' sums in the order of loglik's partials; ||v|| = 0 or max_iter reached: continue from theta2.  alpha = min(-||r|| / ||v||,
 *         -1); theta_x = (theta0 - (2 alpha) r) + (alpha alpha) v in f64, rounded once to f32; F clamped to [eps, hi]; a Q row clamped to
 *         >= eps and divided by its sum, a mode-1 row taken from theta0.  step theta_x -> theta3, lx; continue from theta3 if lx >= l1,
 *         else (a fallback) from theta2.
 *     Cycle-start logliks are therefore non-decreasing up to evaluation error.  Reaching max_iter is GPCA_OK with converged = 0.
 *     info: steps, cycles, converged, fallbacks (the cycles continued from theta2 under accel = 1), loglik = the last cycle-start l0 (the
 *     returned parameters are at least one EM step further on); trace [trace_cap] (the caller's buffer, may be NULL with trace_cap = 0)
 *     receives the first min(trace_cap, cycles) cycle-start logliks.  Q, F and every intermediate stay on the device; per step only
 *     loglik, per cycle also the two norms, come back.
 *  Errors: GPCA_ERR_STATE (no genotypes, a streamed handle, a row-sharded handle, no standardisation, an empty keep mask),
 *     GPCA_ERR_BAD_ARG (a NULL required pointer; K outside 1 .. 16; a mode byte above 2; tol < 0; max_iter < 0; accel or init not 0 or
 *     1; trace NULL with trace_cap > 0; with gpca_admix_step or init = 1, a Q row that is not non-negative and finite with a positive sum
 *     or an F value outside [0, 1]), GPCA_ERR_INVALID_GENOTYPE (a kept row holds a value outside {0, 1, 2, missing} on a sample below N;
 *     the message names the row, as in a12), GPCA_ERR_OOM (checked before any allocation).
 *  Not there: K > 16; restarts from several seeds; projection onto a saved F; standard
 *     errors or bootstrap; haploid and sex chromosomes; ADMIXTURE's own block-relaxation / quasi-Newton numbers; streamed and
 *     row-sharded handles. */
#define GPCA_ADMIX_MAX_K 16
typedef struct gpca_admix_params {
    int32_t K, max_iter;
    uint64_t seed;
    double tol;
    int32_t accel, init;
} gpca_admix_params;
typedef struct gpca_admix_info {
    int64_t steps, cycles;
    int32_t converged, fallbacks;
    double loglik;
    double* trace;        /* in: the caller's buffer [trace_cap], or NULL */
    int64_t trace_cap;    /* in */
} gpca_admix_info;
GPCA_API int gpca_admix_init(gpca_handle* h, int32_t K, uint64_t seed, float* Q /* [N][K] */, float* F /* [Kr][K] */);
GPCA_API int gpca_admix_step(gpca_handle* h, int32_t K, const float* Q, const float* F, const uint8_t* mode /* [N] or NULL */, float* Qn,
                             float* Fn, double* loglik);
GPCA_API int gpca_admix(gpca_handle* h, const gpca_admix_params* params, const uint8_t* mode /* [N] or NULL */, float* Q, float* F,
                        gpca_admix_info* info);

/* ---- a22: the cross-validation error of the admixture fit, and with it the choice of K: a random v-th of the observed calls is hidden
 * from the fit, inside the step's kernel, and scored by its binomial deviance (Alexander & Lange 2011).  Everything of a21 holds as it
 * stands there: the handle's state, the kept rows in PCA-SNP order, Q, F, mode, eps and the summation shape.
 *  Fold of a call: a pure function of (cv_seed, v, the kept-row index i in 0 .. Kr - 1, the sample j); i is the position among the kept
 *     rows, as in a21's F init, not the original row.  w = word i & 3 of philox4x32-10(counter = (j, i >> 2, 0, stream 0x41444D43), key =
 *     (seed low word, seed high word)); fold = ((uint64)w * v) >> 32; 2 <= v <= GPCA_ADMIX_CV_MAX_FOLDS = 64.  Four consecutive kept rows
 *     of a sample share one philox call.  gpca_admix_cv_fold writes that rule for the kept rows [row0, row0 + rows) and the samples 0 ..
 *     N - 1 (host only, no handle: GPCA_ERR_BAD_ARG for out NULL, folds outside 2 .. 64, a negative extent or an index of 2^31 or more).
 *  Hold-out step (v, c): a21's step with every observed call whose fold is c treated as missing: a = b = 0 on the Q side and on the F
 *     side, and no term enters loglik.  Q', F' and loglik are the bits gpca_admix_step returns on the same handle after those calls are
 *     overwritten with the missing code: the same sums in the same order, the held terms absent.  Three more results are evaluated at
 *     the step's input (Q, F) over the held-out observed calls of all samples, whatever their mode:
 *      held_loglik = the sum of g log p1 + (2 - g) log p0 with the same f32 p1, p0 and logf, added in f64 in loglik's order (per sample
 *        over the block's rows, the chunk's 256 samples, the (block, chunk) partials in stride-256 classes);
 *      n_held = the number of held-out observed calls, n_het_held = the number of those with g = 1: exact 64-bit integer counts (integer
 *        atomic adds, whose order cannot matter).
 *  Deviance of fold c: the squared binomial deviance residual of a call with fitted mean 2 p1 is 2 [g log(g / (2 p1)) + (2 - g)
 *     log((2 - g) / (2 p0))]; summed over the fold that is exactly deviance_c = -2 held_loglik_c - 4 ln 2 n_het_held_c (f64, on the host).
 *  cv_error = sum_c deviance_c / sum_c n_held_c, folds ascending; NaN if no call is held.  ADMIXTURE's own fold assignment and printed
 *     digits are not claimed.
 *  gpca_admix_cv: for c = 0 .. v - 1, exactly gpca_admix's loop (a21's cycle rule, SQUAREM, the stop on the training loglik) with the
 *     hold-out step (v, c) in place of the step, from the same start for every fold: init 0 = gpca_admix_init(params->seed), init 1 =
 *     the caller's Q0 and F0, clamped as in a21 (what a supervised fit needs); the caller's mode.  Then one more hold-out step at the
 *     returned parameters, whose Q' and F' are dropped and whose three held-out sums are the fold's score.  out[c]: steps, cycles,
 *     converged, fallbacks, loglik (the last cycle-start training value), held_loglik, n_held, n_het_held, deviance.
 *     The philox init's F uses the row's QC counts over all calls, the held ones included: that is a starting point, not a fit.
 *  Errors: as in a21 (no trace here), and GPCA_ERR_BAD_ARG for folds outside 2 .. 64, fold outside 0 .. folds - 1, Q0 or F0 NULL with
 *     init = 1.
 *  Not there: ADMIXTURE's own fold assignment; standard errors of the CV error; streamed and row-sharded handles. */
#define GPCA_ADMIX_CV_MAX_FOLDS 64
typedef struct gpca_admix_cv_fold_info {
    int64_t steps, cycles;
    int32_t converged, fallbacks;
    double loglik, held_loglik;
    int64_t n_held, n_het_held;
    double deviance;
} gpca_admix_cv_fold_info;
GPCA_API int gpca_admix_cv_fold(uint64_t seed, int32_t folds, int64_t row0, int64_t rows, int64_t N, uint8_t* out /* [rows][N] */);
GPCA_API int gpca_admix_step_holdout(gpca_handle* h, int32_t K, const float* Q, const float* F, const uint8_t* mode /* [N] or NULL */,
                                     int32_t folds, int32_t fold, uint64_t cv_seed, float* Qn, float* Fn, double* loglik, double* held_loglik,
                                     int64_t* n_held, int64_t* n_het_held);
GPCA_API int gpca_admix_cv(gpca_handle* h, const gpca_admix_params* params, const uint8_t* mode /* [N] or NULL */, int32_t folds,
                           uint64_t cv_seed, const float* Q0 /* [N][K], init = 1 */, const float* F0 /* [Kr][K], init = 1 */,
                           gpca_admix_cv_fold_info* out /* [folds] */, double* cv_error);

/* ---- a23: f-statistics (Patterson et al. 2012; ADMIXTOOLS 2's "f2 blocks"): for every jackknife block of SNPs and every pair of a17's
 * groups, the summed unbiased f2 and the number of SNPs behind it, on the device; f2, f3 and f4 with their weighted block-jackknife
 * standard errors and Z scores are linear in those sums and are formed on the host.
 * gpca_f2_blocks: group, P (2 .. GPCA_GROUPS_MAX here) and the kept rows [row0, row1) as in gpca_group_counts.  block [row1 - row0]:
 *     block[r] = the jackknife block of kept row row0 + r, 0 <= block < B, or -1: the row enters nothing.  Any order of block ids is
 *     legal and gives the same result; runs of equal ids are the fast case.  Pair (i, j), j < i, sits at i (i - 1) / 2 + j of
 *     pairs = P (P - 1) / 2, as in gpca_fst_hudson.  For each row with block >= 0 and each pair whose two groups both have n_obs >= 1,
 *     in f64 with no fused multiply-add, in exactly this order (a17's `num`):
 *         n_i = 2 n_obs_i
 *         p_i = (n_het_i + 2 n_hom2_i) / n_i
 *         d   = p_i - p_j
 *         v   = (d d - (p_i (1 - p_i)) / (n_i - 1)) - (p_j (1 - p_j)) / (n_j - 1)
 *         q   = (int64) rint(v 2^40), half to even
 *     acc[block][pair] += q and cnt[block][pair] += 1.  |v| <= 1.5 and the call refuses bands above 2^21 rows, so a call's sums stay
 *     below 2^63.  acc and cnt [B][pairs] are WRITTEN: an untouched entry is 0; the caller adds its bands.  Every sum is an integer, so
 *     any band split, int8 and 2-bit residency, a GPCA_PREC_F32_MFMA handle and any order of the atomics give the same bits.  counts
 *     [rows][P][3], when given, carries the bits of gpca_group_counts for the band: one genotype pass serves a17's files and this.
 *     The sample mask is ignored and no fitted result is touched.
 *  Device: gpca_group_counts' pass as it is, then k_f2_blocks reads the counts workspace once (12 bytes per (row, group)): a workgroup
 *     takes 256 rows in LDS tiles of 32; per tile it forms p_i and (p_i (1 - p_i)) / (n_i - 1) once per (row, group) and a 64-bit
 *     validity mask per row; a thread owns the pairs t, t + 256, ... (at most 8) and keeps their i64 sums and i32 counts in registers
 *     while the block id stays the same; at a block change and at the end of its rows it adds the non-zero counts with one 64-bit and
 *     one 32-bit integer atomic.
 *  Errors: everything on gpca_group_counts' list, and GPCA_ERR_BAD_ARG for a NULL block, acc or cnt, B < 1, a block id outside
 *     -1 .. B - 1 (the message names the row), P < 2, a band above 2^21 rows.  rows = 0 writes zeros and returns GPCA_OK.  GPCA_ERR_OOM
 *     is checked before any allocation and covers block, acc and cnt (B pairs 12 bytes) beside gpca_group_counts' buffers.
 * The two host rules take no handle and work in f64 with no fused multiply-add.
 *  gpca_fstat_blocks: the block of every row of a list of SNPs in genome order.  chrom_change[r] != 0: row r lies on another chromosome
 *     than row r - 1.  A new block starts at row 0, at every chromosome change, and: unit = GPCA_FSTAT_BLOCK_VARIANTS: when the current
 *     block holds `size` rows; unit = GPCA_FSTAT_BLOCK_BP: when pos[r] - (pos of the block's first row) >= size.  block[r] = the number
 *     of blocks started before row r's; *n_blocks = B.  GPCA_ERR_BAD_ARG: rows < 0, size < 1, another unit, NULL n_blocks, and with
 *     rows > 0 a NULL chrom_change or block, or a NULL pos with the bp unit.
 *  gpca_fstat: acc and cnt [B][pairs] = the bands of gpca_f2_blocks added up; quads [M][4] = (a, b, c, d) per statistic, read as
 *         f4(a, b; c, d) = 1/2 [f2(a, d) + f2(b, c) - f2(a, c) - f2(b, d)],  f2(x, x) = 0,
 *     so that f2(A, B) = (A, B, A, B) and f3(C; A, B) = (C, A, C, B).  Per quad:
 *     1. the four terms, each with coefficient +-1/2, are combined into coefficients c_q over distinct unordered pairs; the zero ones
 *        are dropped; the rest are taken in ascending pair index in every sum below.
 *     2. a block is used iff every such pair has cnt >= 1 in it; G = the number of used blocks, taken in ascending order.
 *     3. S_q = sum of acc, C_q = sum of cnt over the used blocks, as integers, converted to f64 once:
 *            theta      = sum_q c_q ((S_q 2^-40) / C_q)
 *            theta_(-b) = sum_q c_q (((S_q - acc_bq) 2^-40) / (C_q - cnt_bq))          (the integer differences converted once)
 *     4. the weighted jackknife (Busing et al. 1999): m_b = sum_q cnt_bq, n = sum_b m_b (integers), h_b = n / m_b,
 *            theta_J = G theta - sum_b ((n - m_b) / n) theta_(-b)
 *            tau_b   = h_b theta - (h_b - 1) theta_(-b)
 *            var     = (1 / G) sum_b ((tau_b - theta_J) (tau_b - theta_J)) / (h_b - 1)
 *     5. out [M][6] = theta, theta_J, se = sqrt(var), z = theta / se, G, min_q C_q.  G < 2: the first four are NaN.  A quad without a
 *        non-zero coefficient, e.g. (A, A, A, A): all six are NaN.
 *     GPCA_ERR_BAD_ARG: NULL acc, cnt or out, NULL quads with M > 0, M < 0, B < 1, P outside 2 .. GPCA_GROUPS_MAX, a quad entry outside
 *     0 .. P - 1.
 *  Where a group has no call on some SNPs, the pairs of one statistic average over different sets of SNPs (a pair counts a SNP iff its
 *     own two groups are observed): the f3 and f4 identities then hold in expectation only, not SNP by SNP.
 *  Not there: D statistics, f4-ratio, qpAdm and qpGraph, normalised f3, blocks in cM (no genetic map: 5 000 kb stands in for 5 cM),
 *     ADMIXTOOLS' own digits, more than GPCA_GROUPS_MAX groups, streamed and row-sharded handles. */
#define GPCA_FSTAT_BLOCK_VARIANTS 0
#define GPCA_FSTAT_BLOCK_BP 1
GPCA_API int gpca_f2_blocks(gpca_handle* h, const int32_t* group /* [N] */, int32_t P, int64_t row0, int64_t row1,
                            const int32_t* block /* [row1 - row0] */, int32_t B, int64_t* acc /* [B][pairs], units of 2^-40, WRITTEN */,
                            int64_t* cnt /* [B][pairs], WRITTEN */, uint32_t* counts /* [rows][P][3] or NULL */);
GPCA_API int gpca_fstat_blocks(const uint8_t* chrom_change /* [rows] */, const int64_t* pos /* [rows]; may be NULL for variants */,
                               int64_t rows, int64_t size, int32_t unit, int32_t* block /* [rows] */, int32_t* n_blocks);
GPCA_API int gpca_fstat(const int64_t* acc, const int64_t* cnt, int32_t B, int32_t P, const int32_t* quads /* [M][4] */, int64_t M,
                        double* out /* [M][6] */);

/* ---- a24: many-trait QTL scan: a12's regression of every kept row of the band against every one of T traits (1 <= T <= 2^20, 0 <= Pc <=
 * 63; the same samples and covariates for all traits), of which only the pairs at or above a threshold and the best row of every trait
 * come back (Matrix eQTL, tensorQTL's trans mode, PheWAS screens).  One wide device pass: no [rows][T] table exists anywhere.
 *  1. host: a12's step 1 on the T columns (a trait column is treated on its own): B_t = (float) Y~_t, Q, yy_t, df = n - Pc - 2.
 *  2. device: n_obs, s1, s2 exact; d_it and e_it with the operands, the sample order and the flush rule of a12's step 2 (a workgroup
 *     owns 128 rows and a strip of trait columns, which it walks in tiles of 64; no split of the sample axis); xb_it = d_it + mbar e_it.
 *     xb_it, xx, sxx and the covariate products behind sxx carry, bit for bit, what gpca_assoc_linear returns for the row and the trait
 *     with the same C and include, whichever traits sit beside it.
 *  3. device, f64, no fused multiply-add: a row is dead if n_obs = 0, xx <= 0 or sxx max_vif < xx; for a live row r2_it = (xb_it xb_it) /
 *     (sxx yy_t); a pair is a hit iff its row is live and r2_it >= r2_min.  A pair with r2 >= 1 (a12's rss <= 0) is still a hit:
 *     gpca_qtl_stats gives it NaN statistics.
 * Outputs: rowinfo [rows][4] as a12 (or NULL); yy [T] (or NULL); hit_count [rows] = the hits of every row, always complete, and
 * *n_found = their sum.  n_found <= cap: hit_index [n_found][2] = (kept row, absolute; trait) and hit_value [n_found][2] = (xb, r2) hold
 * every hit in ascending (row, trait) order.  n_found > cap: the status is still GPCA_OK and the record buffers are unspecified; the
 * caller comes back with a larger buffer or a shorter band (hit_index and hit_value may be NULL iff cap = 0).  best_r2 [t] = the largest
 * r2 of trait t over the band's live rows, best_row [t] = the smallest kept row that attains it; NaN and -1 without a live row (both
 * pointers or neither).  Every output is independent of the launch plan and of the order of any atomic (integer atomics count the hits
 * and place the records, which are sorted before they are returned); a band gives the records of the full call restricted to its rows;
 * int8 and 2-bit residency and a GPCA_PREC_F32_MFMA handle give the same bits; the sample mask is ignored and no fitted result is
 * touched.  GPCA_QTL_TW in the environment (read per call, clamped to a legal strip width: a power of two from 64 to 1024) forces the
 * strip width; it changes no output.  The host step of a call with 256 traits or more runs on GPCA_DESIGN_THREADS threads (default 8; a
 * trait belongs to one thread, so no bit depends on the count).
 * gpca_qtl_stats: the host rule for one hit, out [3] = beta, se, t by a12's step 3 (beta = xb / sxx, rss = yy_t - xb beta, se = sqrt(rss /
 * df / sxx), t = beta / se), all NaN when rss <= 0; gpca_student_t_log10p gives the p-value.
 * Errors: as a12 (GPCA_ERR_STATE: no standardisation, K = 0, a streamed or row-sharded handle; GPCA_ERR_BAD_ARG: T, Pc or the row range
 * out of bounds, a non-finite entry of Y or C on an included sample, df < 1, a constant or collinear column of C, a trait with yy_t = 0
 * (the message names it), max_vif < 1 or not finite; GPCA_ERR_INVALID_GENOTYPE names the row; GPCA_ERR_OOM is checked before any
 * allocation), and GPCA_ERR_BAD_ARG for r2_min outside [0, 1] or NaN, cap < 0, NULL record buffers with cap > 0, NULL hit_count or
 * n_found, only one of best_r2 / best_row.
 * Not there (cis windows and permutation p-values are section a25): per-trait sample sets and missing phenotypes, interaction terms,
 * case / control traits, bf16 or other reduced-precision operands, streamed and row-sharded handles. */
GPCA_API int gpca_assoc_qtl(gpca_handle* h, const double* Y /* [N][T] */, int64_t T, const double* C /* [N][Pc] or NULL */, int32_t Pc,
                            const uint8_t* include /* [N] or NULL */, double max_vif, double r2_min, int64_t row0, int64_t row1,
                            double* rowinfo /* [rows][4] or NULL */, double* yy /* [T] or NULL */, uint32_t* hit_count /* [rows] */,
                            uint32_t* hit_index /* [cap][2]; NULL iff cap = 0 */, double* hit_value /* [cap][2] */, int64_t cap,
                            int64_t* n_found, double* best_r2 /* [T] or NULL */, int64_t* best_row /* [T] or NULL */);
GPCA_API void gpca_qtl_stats(double xb, double sxx, double yy_t, double df, double* out /* [3] */);
/* the smallest t >= 0 whose two-sided -log10 p at df degrees of freedom (gpca_student_t_log10p) reaches log10p, by bisection down to
 * neighbouring doubles: the cutoff a threshold on the p-value becomes (r2_min = t^2 / (t^2 + df)).  0 for log10p <= 0, NaN for NaN or
 * df <= 0, +inf when no finite t reaches it.  Host only. */
GPCA_API double gpca_qtl_t_min(double log10p, double df);

/* ---- a25: cis-QTL mapping: for each of G traits the best kept row of its own window [lo, hi) and the null distribution of that best
 * r2 under P permutations of the trait (FastQTL, tensorQTL's cis mode).  Inputs as a24 (Y [N][G], C [N][Pc], include, max_vif), plus
 * win [G][2] = [lo, hi) in kept rows, 0 <= lo <= hi <= K, and perm [P][n] u32, 0 <= P <= 65 535, n = the included samples: every row a
 * permutation of 0 .. n - 1 over the included samples in ascending sample order; one table serves every trait of the call.
 *  1. host: a12's step 1 once on the G columns: the residuals b_t (f64, over the included samples), the orthonormal covariate basis Q,
 *     yy_t, df = n - Pc - 2.
 *  2. device: the per-row pass of a24 (sums, rowinfo) once over the union of the windows.
 *  3. the panel of trait t, P + 1 columns in a24's layout.  Column 0 is (float) b_t: the bits a24 stages.  Column p + 1 is the permuted
 *     residual taken back into the covariates' complement, on the device in f64 without fused multiply-add:
 *       v_i = b_t[perm[p][i]];  c_j = sum_i Q_ij v_i, i ascending, one running sum;  s_i = sum_j Q_ij c_j, j ascending, one running
 *       sum;  the value is (float)(v_i - s_i).  Q is the basis of step 1 as it stands (its columns are centred: there is no intercept
 *     column).  With Pc = 0 the value is (float) v_i.  yy of every permuted column is yy_t (the unpermuted residual's norm: FastQTL's rule).
 *  4. a24's steps 2 and 3 on the kept rows [lo, hi) and all P + 1 columns, with the same liveness rule: xb, xx, sxx carry
 *     gpca_assoc_linear's bits, r2 = (xb xb) / (sxx yy_t) in f64; per column the largest r2 over the live rows, the smallest row on a tie.
 * Outputs per trait: n_var = the live rows of the window; best_row, best_r2 and best_stat [3] = (xb, sxx, yy_t) of column 0's best row
 * (gpca_qtl_stats applies directly); perm_r2 [P] = the best r2 of every permuted column.  A window without a live row: n_var = 0,
 * best_row = -1, NaN everywhere else.  Every output of a trait is a function of that trait, its window, the table, C and include alone:
 * not of the other traits of the call or their order, not of the launch plan (GPCA_QTL_TW is honoured as in a24), not of int8 / 2-bit
 * residency or a GPCA_PREC_F32_MFMA handle.  No atomic anywhere.
 * Errors: as a24, plus GPCA_ERR_BAD_ARG for a window outside [0, K] or with lo > hi (the message names the trait), for P out of range,
 * for perm = NULL or perm_r2 = NULL with P > 0, and for a table row that is not a permutation (checked on the host; the message names the
 * row); GPCA_ERR_STATE for streamed and row-sharded handles.
 * gpca_qtl_perm_panel: step 3 alone on the caller's b [n] and Q [n][Pc] (row-major): out [P][n] = the columns 1 .. P.  Needs no genotypes.
 * gpca_qtl_perm_table (host only, a pure function): row p starts as 0 .. n - 1; for step s = 0 .. n - 2, with i = n - 1 - s: r = word
 *   s & 3 of philox4x32-10(counter = (s >> 2, p, 0, 0x51544C50), key = (seed low word, seed high word)); j = ((uint64) r (i + 1)) >> 32;
 *   the entries i and j change places (Fisher-Yates with a multiply-shift index).
 * gpca_qtl_beta_approx (host only): FastQTL's beta approximation.  With p(r2, d) = the two-sided Student p-value of t^2 = d r2 / (1 - r2)
 *   at d degrees of freedom (gpca_student_t_log10p): NaN entries of perm_r2 drop out, P' are left.
 *   (a) pval_perm = (1 + #{perm_r2 >= r2_nominal}) / (P' + 1).  With P' < 10 every other field is NaN.
 *   (b) true_df = the root in d of log shape1_mom(d) = 0, where shape1_mom = m (m (1 - m) / v - 1) from the mean m and the variance v
 *       (divisor P' - 1) of p(perm_r2, d): bisection on [1, 2 df] down to an interval of 1e-6 df, its midpoint.  No sign change: d = df
 *       and status bit 1.
 *   (c) shape1, shape2 = the maximum-likelihood Beta fit of p(perm_r2, true_df): Newton with step halving on psi(a) - psi(a + b) =
 *       mean log p, psi(b) - psi(a + b) = mean log(1 - p), started at the moment estimates.  On failure: the moment estimates and status
 *       bit 2.
 *   (d) log10p_nominal_true = -log10 p(r2_nominal, true_df).
 *   (e) log10p_beta = -log10 I_x(shape1, shape2) at x = p(r2_nominal, true_df): the continued fraction, assembled in log space from
 *       log x, so it does not underflow.
 *   out [7] = pval_perm, true_df, shape1, shape2, log10p_nominal_true, log10p_beta, the moment estimate of shape1.  All NaN for a NaN
 *   r2_nominal or df < 1.
 * The P.qtl.cis file of the command lines (io.write_qtl_cis, formats.hpp QtlCisWriter): one line per trait; a trait without a position
 * is `TRAIT` and 15 `NA`; a trait with n_var = 0 keeps what is known of it, `TRAIT CHROM POS 0`, and has `NA` in the 12 columns from ID on.
 * Not there: conditionally independent signals, q-values across traits, per-trait sample sets, interaction terms, adaptive permutation
 * counts, grouped phenotypes, tensorQTL's or FastQTL's own digits, streamed and row-sharded handles. */
GPCA_API int gpca_assoc_qtl_cis(gpca_handle* h, const double* Y /* [N][G] */, int64_t G, const double* C /* [N][Pc] or NULL */, int32_t Pc,
                                const uint8_t* include /* [N] or NULL */, double max_vif, const int64_t* win /* [G][2] */,
                                const uint32_t* perm /* [P][n]; NULL iff P = 0 */, int32_t P, int64_t* n_var /* [G] */,
                                int64_t* best_row /* [G] */, double* best_r2 /* [G] */, double* best_stat /* [G][3] */,
                                double* perm_r2 /* [G][P]; NULL iff P = 0 */);
GPCA_API int gpca_qtl_perm_panel(gpca_handle* h, const double* b /* [n] */, const double* Q /* [n][Pc] */, int32_t Pc, int64_t n,
                                 const uint32_t* perm /* [P][n] */, int32_t P, float* out /* [P][n] */);
GPCA_API int gpca_qtl_perm_table(uint64_t seed, int64_t n, int32_t P, uint32_t* out /* [P][n] */);
GPCA_API int gpca_qtl_beta_approx(const double* perm_r2 /* [P] */, int64_t P, double r2_nominal, double df, double* out /* [7] */,
                                  int32_t* status /* or NULL */);

/* ---- f3: the stages of EigenSNPCoreAlgorithm::compute_pca (main.rs:311-327, 359-366) ------------------------------------------
 * The algorithm lives in the un-vendored efficient_pca crate (Cargo.toml:30, branch "main", no pinned revision): what follows is
 * the stage structure of its published description -- per-LD-block local bases learnt on a sample subset, condensed features of
 * all samples, row standardisation, an initial global randomized PCA of the condensed features, refinement passes on the full
 * matrix -- with every pass over the genotypes on the device.  Parity with the crate is UNPINNED (no source, no golden vectors);
 * the host mirror (EigenSNPCoreAlgorithm.compute_pca, local_stage = True) drives these calls and is checked against a numpy
 * restatement of the same stages and against exact PCA.
 *
 * gpca_copy_rows: dst (same device and storage mode) receives rows [row0, row0 + rows) of src's RESIDENT matrix, device to device:
 *   an LD block as a matrix of its own (follow with gpca_set_standardization on dst).
 * gpca_set_sample_mask: mask[n] != 0 = sample n takes part in learning the basis; gpca_rsvd then learns scores / loadings from
 *   those columns only (its eigenvalues are variances over the subset: / (subset size - 1)), gpca_transform still projects every
 *   sample.  NULL clears.
 * gpca_set_condensed_basis: W[i][0..cmax) = SNP row i's coefficients (local loading / feature s.d.) on the condensed features
 *   [feat0[i], feat0[i] + cmax) of its block, zero-padded; feat0[i] < 0 = in no block; R = number of condensed features.
 * gpca_rsvd_condensed: randomized PCA of the row-standardised condensed feature matrix C* = W^T A (R x N, never formed: its
 *   products run through the genotype GEMMs).  Leaves N x k sample scores and C*'s eigenvalues; no loadings.
 * gpca_refine: one refinement pass from sample scores S0 [N][k]: L = orth(A S0), S = A^T L, S^T S = W Sigma^2 W^T;
 *   scores = S W, loadings = L W, eigenvalues = Sigma^2 / (N - 1), through the usual getters. */
GPCA_API int gpca_copy_rows(gpca_handle* dst, gpca_handle* src, int64_t row0, int64_t rows);
GPCA_API int gpca_set_sample_mask(gpca_handle* h, const uint8_t* mask /* [N] or NULL */);
GPCA_API int gpca_set_condensed_basis(gpca_handle* h, const float* W /* [M][cmax] */, const int32_t* feat0 /* [M] */, int32_t cmax, int64_t R);
GPCA_API int gpca_rsvd_condensed(gpca_handle* h, int32_t k, int32_t oversample, int32_t power_iters, uint64_t seed);
GPCA_API int gpca_refine(gpca_handle* h, const double* S0 /* [N][k] */, int32_t k);

/* ---- e: SNP-row sharding across GPUs ------------------------------------------------------- */
#define GPCA_UNIQUE_ID_BYTES 128
GPCA_API int gpca_comm_get_unique_id(void* out_id /* GPCA_UNIQUE_ID_BYTES */);
/* This handle holds rows [snp_offset, snp_offset + M) of a matrix sharded over `world` ranks.
 * Creates an RCCL communicator; the N x l sketch and l x l Gram blocks are all-reduced. */
GPCA_API int gpca_comm_init(gpca_handle* h, int32_t world, int32_t rank, const void* unique_id, int64_t snp_offset);
/* Host-staged all-reduce hook (sum, in place, f64) used instead of RCCL when set: lets any
 * transport (MPI, gloo) carry the exchange; also how the CPU tests exercise the N>1 path.  Called with the handle's lock held
 * (other handles -- the peers' -- are unaffected). */
typedef int (*gpca_allreduce_fn)(void* user, double* host_buf, int64_t count);
GPCA_API int gpca_set_allreduce_hook(gpca_handle* h, gpca_allreduce_fn fn, void* user, int32_t world,
                            int32_t rank, int64_t snp_offset);

/* How many ranks the handle's exchange actually reaches: a 1.0 per rank summed through the same transport as the sketch (RCCL
 * communicator or hook).  Collective: every rank of the sharded matrix must call it.  1 for an unsharded handle. */
GPCA_API int gpca_comm_count_ranks(gpca_handle* h, int32_t* ranks);

/* ---- d: measurement ------------------------------------------------------------------------- */
typedef struct gpca_kernel_timing {
    char name[32];
    int64_t launches;
    double total_ms;   /* sum of HIP-event durations on the engine's stream */
    double flops;      /* algorithmic (un-padded) flops summed over those launches */
    double bytes;      /* algorithmic HBM bytes summed over those launches */
} gpca_kernel_timing;
/* Timings are OFF by default (gpca_enable_timings(h, 1) turns them on; n > 1: only every n-th gpca_rsvd call records its events -- a
 * recorded event pair costs the stream about 5 us of idle time, which a caller who wants per-kernel figures of a long run need not
 * pay on every call: launches / total_ms then cover the sampled calls only); records are folded into per-name totals
 * once 32768 are pending, so a long-running host never accumulates events.
 * Timings accumulated since the last gpca_reset_timings (events resolved lazily here). */
GPCA_API int gpca_get_timings(gpca_handle* h, gpca_kernel_timing* out, int32_t cap, int32_t* n);
GPCA_API int gpca_reset_timings(gpca_handle* h);
GPCA_API int gpca_enable_timings(gpca_handle* h, int32_t on);
GPCA_API int gpca_synchronize(gpca_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* GPCA_H */
