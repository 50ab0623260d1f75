"""Host-side mirror of the reference's operator interface for the hot path, over the C ABI.

The reference is Rust; this image has no Rust toolchain, so the host side above
``include/gpca.h`` is written here with the reference's names and argument meaning:

===============================  =====================================================
reference (file:line)            here
===============================  =====================================================
PCA::new/rfit/transform          :class:`PCA`                       main.rs:602,648-660
PcaReadyGenotypeAccessor trait   :class:`MicroarrayGenotypeAccessor` prepare.rs:1838-2030
PcaSnpId / QcSampleId            plain ints (dense 0-based)          prepare.rs:1485,1854,1858
LdBlockSpecification             :class:`LdBlockSpecification`       prepare.rs:1540-1543
EigenSNPCoreAlgorithmConfig      :class:`EigenSNPCoreAlgorithmConfig` main.rs:311-327
EigenSNPCoreAlgorithm            :class:`EigenSNPCoreAlgorithm`      main.rs:359-366
===============================  =====================================================

Everything numeric happens in libgpca.so on the GPU; numpy is only the host buffer type.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import GpcaError


def _vp(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _band_entries(row0: int, row1: int, diag: bool) -> int:
    """Entries of the rows [row0, row1) of the lower triangle packed row-major, with or without the diagonal (plan_math.h: band_entries)."""
    return max(row1 * (row1 + 1) // 2 - row0 * (row0 + 1) // 2 if diag else row1 * (row1 - 1) // 2 - row0 * (row0 - 1) // 2, 0)


def _band_to_full(band: np.ndarray, N: int, diag: bool, fill=0) -> np.ndarray:
    """The full symmetric [N][N] (+ band's trailing dimensions) array of a packed band that holds every row; `fill` where the band has
    no entry (the diagonal of a band without one)."""
    il = np.tril_indices(N, 0 if diag else -1)
    full = np.full((N, N) + band.shape[1:], fill, band.dtype)
    full[il] = band
    full.swapaxes(0, 1)[il] = band
    return full


@dataclass
class QcConfig:
    """MicroarrayDataPreparerConfig thresholds; defaults = clap's effective ones (main.rs:545-560)."""
    min_snp_call_rate: float = 0.98
    min_snp_maf: float = 0.01
    max_snp_hwe_p_value: float = 1e-6

    @staticmethod
    def none() -> "QcConfig":
        return QcConfig(0.0, 0.0, 1.0)


class PanelSource:
    """``gpca_panel_source``: where the SNP rows of a matrix come from, panel by panel.

    * ``PanelSource.host_i8(fn)``  -- ``fn(row0, rows) -> int8 [rows, N]`` (0/1/2, -127 missing)
    * ``PanelSource.host_bed(fn)`` -- ``fn(row0, rows) -> uint8 [rows, ceil(N/4)]`` PLINK .bed rows
    * ``PanelSource.synth(thresh, seed, snp_offset)`` / ``.synth16(...)`` -- device generators

    Used for resident loading (``GpcaEngine.load_from_source``) and for out-of-core streaming
    (``GpcaEngine.stream_open``; BASELINE.json configs[4]).  The reference's analogue is the accessor's strip pull loop
    (main.rs:322,584; prepare.rs:1839-2022)."""

    def __init__(self, kind: int, fill=None, thresh: Optional[np.ndarray] = None, seed: int = 0, snp_offset: int = 0,
                 mapped: Optional[np.ndarray] = None, flags: int = 0):
        self.kind = kind
        self.mapped, self.flags = mapped, int(flags)
        self.thresh = None if thresh is None else np.ascontiguousarray(thresh, np.uint32)
        self.seed, self.snp_offset = int(seed), int(snp_offset)
        self._fill = fill
        self._cb = _lib.PANEL_FN(self._tramp) if fill is not None else _lib.PANEL_FN()
        self.error: Optional[BaseException] = None

    def _tramp(self, _user, row0, rows, dst, ld):
        try:
            a = np.asarray(self._fill(int(row0), int(rows)))
            want = np.int8 if self.kind == _lib.PANEL_HOST_I8 else np.uint8
            if a.dtype != want or a.shape != (rows, ld):
                raise ValueError(f"panel callback must return {np.dtype(want).name} [{rows}, {ld}], got {a.dtype} {a.shape}")
            view = np.ctypeslib.as_array(C.cast(dst, C.POINTER(C.c_uint8)), shape=(rows, ld))
            view[...] = a.view(np.uint8)
            return 0
        except BaseException as e:  # noqa: BLE001 -- reported through the C status
            self.error = e
            return 1

    def c_struct(self) -> "_lib.gpca_panel_source":
        st = _lib.gpca_panel_source()
        st.kind = self.kind
        st.fill = self._cb
        st.seed, st.snp_offset = self.seed, self.snp_offset
        if self.thresh is not None:
            st.n_pop = self.thresh.shape[1]
            st.thresh = self.thresh.ctypes.data_as(C.c_void_p)
        if self.mapped is not None:
            st.user = self.mapped.ctypes.data_as(C.c_void_p)
            st.host_ld = self.mapped.strides[0]
        st.flags = self.flags
        return st

    @staticmethod
    def host_i8(fn):
        return PanelSource(_lib.PANEL_HOST_I8, fill=fn)

    @staticmethod
    def host_bed(fn):
        return PanelSource(_lib.PANEL_HOST_BED, fill=fn)

    @staticmethod
    def _mapped(kind, a, want, register):
        a = np.asarray(a)
        if a.dtype != want or a.ndim != 2 or (a.shape[1] > 1 and a.strides[1] != 1) or a.strides[0] < a.shape[1]:
            raise ValueError(f"mapped panel source: a 2-D {np.dtype(want).name} array with contiguous rows is required")
        return PanelSource(kind, mapped=a, flags=_lib.SOURCE_REGISTER if register else 0)

    @staticmethod
    def mapped_i8(a, register=False):
        """The whole int8 matrix [M, N] in host memory (an ndarray or np.memmap; rows contiguous, any row pitch): no callback, the
        library's copy threads stage the panels -- or, register=True, the pages are locked once and DMA-ed in place."""
        return PanelSource._mapped(_lib.PANEL_MAPPED_I8, a, np.int8, register)

    @staticmethod
    def mapped_bed(a, register=False):
        """The .bed payload [M, ceil(N/4)] uint8 in host memory (e.g. np.memmap of the file past its 3-byte magic)."""
        return PanelSource._mapped(_lib.PANEL_MAPPED_BED, a, np.uint8, register)

    @staticmethod
    def synth(thresh, seed, snp_offset=0):
        return PanelSource(_lib.PANEL_SYNTH, thresh=thresh, seed=seed, snp_offset=snp_offset)

    @staticmethod
    def synth16(thresh16, seed, snp_offset=0, bench_hold=False):
        """bench_hold: MEASUREMENT ONLY (gpca.h GPCA_SOURCE_BENCH_HOLD): buffers that hold a generated panel are not generated again."""
        return PanelSource(_lib.PANEL_SYNTH16, thresh=thresh16, seed=seed, snp_offset=snp_offset, flags=_lib.SOURCE_BENCH_HOLD if bench_hold else 0)


# Defaults added to every GpcaEngine's gpca_config.reserved (flags OR-ed in, wave targets used when the caller passes 0).  The library
# itself reads no environment variable for its kernel choice; a harness that wants every engine of a run on, say, the reference
# kernels sets these (the parity tests do, through monkeypatch.setattr).
DEFAULT_FLAGS = 0
DEFAULT_GQ_WAVES = 0
DEFAULT_GTT_WAVES = 0


class GpcaEngine:
    """One opaque ``gpca_handle``: one GPU, one SNP-row shard of the genotype matrix.

    Default = the exact-integer GEMM path on int8-resident genotypes (``PREC_I8_EXACT`` / ``STORE_INT8``), the path
    bench.py's headline times; ``PREC_F32_MFMA`` selects the f32 matrix-core path, ``STORE_2BIT`` packed residency."""

    def __init__(self, device: int = -1, precision: int = _lib.PREC_I8_EXACT, storage: int = _lib.STORE_INT8,
                 digit_planes: int = 0, flags: int = 0, gq_waves: int = 0, gtt_waves: int = 0):
        """flags: _lib.CFG_* bits of gpca_config.reserved[0]; gq_waves / gtt_waves: grid targets of the two GEMMs (0 = tuned defaults)."""
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self._device, self.precision, self.storage, self.digit_planes = device, precision, storage, digit_planes
        cfg = _lib.gpca_config(device=device, precision=precision, storage=storage, digit_planes=digit_planes)
        cfg.reserved[0], cfg.reserved[1], cfg.reserved[2] = flags | DEFAULT_FLAGS, gq_waves or DEFAULT_GQ_WAVES, gtt_waves or DEFAULT_GTT_WAVES
        rc = self._lib.gpca_create(C.byref(cfg), C.byref(self._h))
        if rc != _lib.GPCA_OK:
            raise GpcaError(rc, self._lib.gpca_last_error(None).decode())
        self._hook_ref = None
        self._source_ref = None

    # -- plumbing
    def _chk(self, rc: int):
        if rc != _lib.GPCA_OK:
            src = self._source_ref[0] if self._source_ref else None
            if src is not None and src.error is not None:      # a panel callback raised: show its exception
                err, src.error = src.error, None
                raise err
            raise GpcaError(rc, self._lib.gpca_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.gpca_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- residency
    def upload_genotypes_i8(self, snp_major: np.ndarray):
        """int8 [M, N] SNP-major dosages (0/1/2, -127 missing)."""
        g = np.asarray(snp_major)
        if g.dtype != np.int8 or g.ndim != 2:
            raise ValueError("snp_major must be a 2-D int8 array [SNPs, samples]")
        if g.strides[1] != 1:
            g = np.ascontiguousarray(g)
        self._chk(self._lib.gpca_upload_genotypes_i8(self._h, _vp(g), g.shape[0], g.shape[1], g.strides[0]))

    def upload_bed2bit(self, bed_rows: np.ndarray, n_samples: int):
        b = np.ascontiguousarray(bed_rows, np.uint8)
        if b.ndim != 2 or b.shape[1] != (n_samples + 3) // 4:
            raise ValueError("bed_rows must be uint8 [SNPs, ceil(N/4)]")
        self._chk(self._lib.gpca_upload_bed2bit(self._h, _vp(b), b.shape[0], n_samples))

    def synth_genotypes(self, M: int, N: int, seed: int, thresh: np.ndarray, snp_offset: int = 0):
        t = np.ascontiguousarray(thresh, np.uint32)
        if t.shape[0] != M:
            raise ValueError("thresh must be uint32 [M, P]")
        self._chk(self._lib.gpca_synth_genotypes(self._h, M, N, seed, _vp(t), t.shape[1], snp_offset))

    def load_from_source(self, src: "PanelSource", M: int, N: int):
        """Resident load through a panel source, chunked through bounded staging."""
        cs = src.c_struct()
        if src.thresh is not None and src.thresh.shape[0] != M:
            raise ValueError("thresh must be uint32 [M, P]")
        rc = self._lib.gpca_load_from_source(self._h, C.byref(cs), M, N)
        if rc != _lib.GPCA_OK and src.error is not None:
            raise src.error
        self._chk(rc)

    def stream_open(self, src: "PanelSource", M: int, N: int, panel_rows: int = 0, ring_slots: int = 3, fused: bool = True,
                    cache_bytes: int = 0):
        """Out-of-core mode: later snp_stats / rsvd / transform calls walk the matrix panel by panel through a ring of
        HBM buffers (the source object must outlive them; it is kept referenced here).  fused = True: a power iteration
        reads every panel once (4 passes per rsvd at q = 2); False: 6 passes, bit-identical to the resident engine.
        cache_bytes: HBM for the panel cache (stream_set_cache; -1 = what is free, 0 = none)."""
        cs = src.c_struct()
        if src.thresh is not None and src.thresh.shape[0] != M:
            raise ValueError("thresh must be uint32 [M, P]")
        self._source_ref = (src, cs)
        self._chk(self._lib.gpca_stream_open(self._h, C.byref(cs), M, N, panel_rows, ring_slots))
        self._chk(self._lib.gpca_stream_set_fused(self._h, int(fused)))
        if cache_bytes:
            self.stream_set_cache(cache_bytes)

    def stream_info(self) -> dict:
        """gpca_stream_get_info: shape of the open panel stream and where its host-side time went."""
        info = _lib.gpca_stream_info()
        self._chk(self._lib.gpca_stream_get_info(self._h, C.byref(info)))
        return {k: getattr(info, k) for k, _ in info._fields_ if k != "reserved"}

    def stream_set_cache(self, max_bytes: int = -1) -> int:
        """Keep the leading panels in spare HBM (asked of the source once, read in place afterwards); returns how many."""
        n = C.c_int32()
        self._chk(self._lib.gpca_stream_set_cache(self._h, int(max_bytes), C.byref(n)))
        return n.value

    def device_memory(self):
        """(free, total) bytes of the engine's device."""
        f, t = C.c_int64(), C.c_int64()
        self._chk(self._lib.gpca_get_device_memory(self._h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def download_genotypes_i8(self) -> np.ndarray:
        M, N = self.dims()
        out = np.empty((M, N), np.int8)
        self._chk(self._lib.gpca_download_genotypes_i8(self._h, _vp(out), N))
        return out

    def storage_in_use(self):
        """(storage, precision) the handle runs with: STORE_AUTO resolves to STORE_2BIT / STORE_INT8 when the genotypes arrive."""
        st, pr = C.c_int32(), C.c_int32()
        self._chk(self._lib.gpca_get_storage(self._h, C.byref(st), C.byref(pr)))
        return st.value, pr.value

    def dims(self):
        M, N = C.c_int64(), C.c_int64()
        self._chk(self._lib.gpca_dims(self._h, C.byref(M), C.byref(N)))
        return M.value, N.value

    # -- a1 / a3
    def snp_stats(self, qc: Optional[QcConfig] = None, fetch: bool = True):
        M, _ = self.dims()
        q = qc or QcConfig.none()
        cq = _lib.gpca_qc_config(q.min_snp_call_rate, q.min_snp_maf, q.max_snp_hwe_p_value)
        if not fetch:
            self._chk(self._lib.gpca_snp_stats(self._h, C.byref(cq), None, None, None))
            return None
        mu = np.empty(M, np.float32); sg = np.empty(M, np.float32); keep = np.empty(M, np.uint8)
        self._chk(self._lib.gpca_snp_stats(self._h, C.byref(cq), _vp(mu), _vp(sg), _vp(keep)))
        return dict(mu=mu, sigma=sg, keep=keep)

    def snp_qc_detail(self):
        M, _ = self.dims()
        counts = np.empty((M, 4), np.uint32); reason = np.empty(M, np.uint8)
        self._chk(self._lib.gpca_get_snp_qc_detail(self._h, _vp(counts), _vp(reason)))
        return counts, reason

    def set_standardization(self, mu, sigma, keep=None):
        mu = np.ascontiguousarray(mu, np.float32); sigma = np.ascontiguousarray(sigma, np.float32)
        keep = None if keep is None else np.ascontiguousarray(keep, np.uint8)
        self._chk(self._lib.gpca_set_standardization(self._h, _vp(mu), _vp(sigma), _vp(keep)))

    def get_standardization(self):
        M, _ = self.dims()
        mu = np.empty(M, np.float32); sg = np.empty(M, np.float32); keep = np.empty(M, np.uint8)
        self._chk(self._lib.gpca_get_standardization(self._h, _vp(mu), _vp(sg), _vp(keep)))
        return dict(mu=mu, sigma=sg, keep=keep)

    @staticmethod
    def hwe_chi_squared_p_value(n_hom1: int, n_het: int, n_hom2: int) -> float:
        """prepare.rs:1641-1745 (host helper in libgpca.so)."""
        return float(_lib.load().gpca_hwe_chi_squared_p_value(int(n_hom1), int(n_het), int(n_hom2)))

    # -- a2
    def standardize_block(self, pca_snp_ids: Sequence[int], qc_sample_ids: Sequence[int]) -> np.ndarray:
        s = np.ascontiguousarray(pca_snp_ids, np.int64); c = np.ascontiguousarray(qc_sample_ids, np.int64)
        out = np.zeros((len(s), len(c)), np.float32)
        self._chk(self._lib.gpca_standardize_block(self._h, _vp(s), len(s), _vp(c), len(c), _vp(out)))
        return out

    def num_pca_snps(self) -> int:
        return int(self._lib.gpca_num_pca_snps(self._h))

    def num_qc_samples(self) -> int:
        return int(self._lib.gpca_num_qc_samples(self._h))

    def pca_snp_rows(self) -> np.ndarray:
        rows = np.empty(self.num_pca_snps(), np.int64)
        self._chk(self._lib.gpca_get_pca_snp_rows(self._h, _vp(rows)))
        return rows

    # -- a5 / a6
    def rsvd(self, k: int, oversample: int = 10, power_iters: int = 2, seed: int = 1):
        self._chk(self._lib.gpca_rsvd(self._h, k, oversample, power_iters, seed))
        self._k, self._l = k, k + oversample

    def scores(self, f64: bool = False) -> np.ndarray:
        _, N = self.dims()
        out = np.empty((N, self._k), np.float64 if f64 else np.float32)
        fn = self._lib.gpca_get_scores_f64 if f64 else self._lib.gpca_get_scores
        self._chk(fn(self._h, _vp(out)))
        return out

    def eigenvalues(self) -> np.ndarray:
        out = np.empty(self._k, np.float64)
        self._chk(self._lib.gpca_get_eigenvalues(self._h, _vp(out)))
        return out

    def singular_values(self) -> np.ndarray:
        out = np.empty(self._l, np.float64)
        self._chk(self._lib.gpca_get_singular_values(self._h, _vp(out)))
        return out

    def loadings(self) -> np.ndarray:
        out = np.empty((self.num_pca_snps(), self._k), np.float32)
        self._chk(self._lib.gpca_get_loadings(self._h, _vp(out)))
        return out

    def transform(self) -> np.ndarray:
        _, N = self.dims()
        out = np.empty((N, self._k), np.float64)
        self._chk(self._lib.gpca_transform(self._h, _vp(out)))
        return out

    def project(self, mu: np.ndarray, sigma: np.ndarray, W: np.ndarray):
        """Scores of this engine's genotypes on a fitted model (gpca_project): mu, sigma [M], W [M][k] in this engine's row order,
        zero rows = not in the model.  Missing calls are mean-imputed.  Returns (scores f64 [N][k], n_used int32 [N])."""
        M, N = self.dims()
        mu = np.ascontiguousarray(mu, np.float32); sigma = np.ascontiguousarray(sigma, np.float32)
        W = np.ascontiguousarray(W, np.float32)
        if W.ndim == 1:
            W = W.reshape(-1, 1)
        if mu.shape != (M,) or sigma.shape != (M,) or W.ndim != 2 or W.shape[0] != M:
            raise ValueError(f"project: mu and sigma must be [{M}] and W [{M}][k]")
        k = W.shape[1]
        scores = np.empty((N, k), np.float64)
        used = np.empty(N, np.int32)
        self._chk(self._lib.gpca_project(self._h, _vp(mu), _vp(sigma), _vp(W), k, _vp(scores), _vp(used)))
        return scores, used

    def grm(self, scaling: str = "standardized", rows: Optional[Tuple[int, int]] = None, npairs: bool = False):
        """Genetic relationship matrix of the kept rows (gpca_grm): (1 / K) Z^T Z with missing calls at 0, K = kept rows.
        scaling: "standardized" (Z = r g + b, the matrix gpca_rsvd factorises) or "centred" (Z = g - mu).  rows = (row0, row1): rows
        [row0, row1) of the lower triangle packed row-major (GCTA .grm.bin order), f64; rows = None: the full symmetric [N][N] f64 array.
        npairs=True also returns the number of kept rows where both samples are observed (f32, same shape)."""
        if scaling not in ("standardized", "centred"):
            raise ValueError('scaling must be "standardized" or "centred"')
        sc = _lib.GRM_STANDARDIZED if scaling == "standardized" else _lib.GRM_CENTRED
        N = self.dims()[1]
        r0, r1 = (0, N) if rows is None else (int(rows[0]), int(rows[1]))
        E = _band_entries(r0, r1, True)
        g = np.empty(max(E, 1), np.float64)
        npv = np.empty(max(E, 1), np.float32) if npairs else None
        self._chk(self._lib.gpca_grm(self._h, sc, r0, r1, _vp(g), _vp(npv)))
        g = g[:E]
        npv = npv[:E] if npairs else None
        if rows is not None:
            return (g, npv) if npairs else g
        full = _band_to_full(g, N, True)
        return (full, _band_to_full(npv, N, True)) if npairs else full

    def king(self, rows: Optional[Tuple[int, int]] = None, counts: bool = False):
        """KING-robust kinship of the kept rows (gpca_king).  rows = (row0, row1): rows [row0, row1) of the STRICTLY lower triangle packed
        row-major (pair (j, k < j) at j (j - 1) / 2 - row0 (row0 - 1) / 2 + k), f64; rows = None: the full symmetric [N][N] f64 array with
        0.5 on the diagonal.  NaN where a pair has no het call on the rows both samples are called on.  counts=True also returns the
        int32 counts NSNP, HETHET, IBS0 per pair ([pairs][3], or [N][N][3] with zeros on the diagonal)."""
        N = self.dims()[1]
        r0, r1 = (0, N) if rows is None else (int(rows[0]), int(rows[1]))
        E = _band_entries(r0, r1, False)
        k = np.empty(max(E, 1), np.float64)
        cnt = np.empty((max(E, 1), 3), np.int32) if counts else None
        self._chk(self._lib.gpca_king(self._h, r0, r1, _vp(k), _vp(cnt)))
        k = k[:E]
        cnt = cnt[:E] if counts else None
        if rows is not None:
            return (k, cnt) if counts else k
        full = _band_to_full(k, N, False, fill=0.5)
        return (full, _band_to_full(cnt, N, False)) if counts else full

    def ld_window(self, win_end, wmax: Optional[int] = None, rows: Optional[Tuple[int, int]] = None, threshold: Optional[float] = None,
                  r2: bool = True, counts: bool = False):
        """Windowed LD of the kept rows (gpca_ld_window), rows in PCA-SNP order.  win_end[t]: row row0 + t is paired with every later
        kept row below win_end[t]; slot d = j - i - 1.  rows = (row0, row1), default every kept row; wmax: slots per row, default the
        widest window of win_end (at least 1).  Returns a dict with the outputs asked for: "r2" [rows][wmax] f64 (NaN where a row of the
        pair has no variance over the jointly observed samples), "counts" [rows][wmax][6] int32 = n, sx, sy, sxx, syy, sxy, and, when a
        threshold is given, "above" [rows][ceil(wmax / 64)] uint64 (bit d % 64 of word d / 64 = r2 > threshold).  Slots outside a row's
        window are 0."""
        K = int(self._lib.gpca_num_pca_snps(self._h))
        r0, r1 = (0, K) if rows is None else (int(rows[0]), int(rows[1]))
        we = np.ascontiguousarray(win_end, np.int64)
        n = max(r1 - r0, 0)
        if we.shape != (n,):
            raise ValueError("win_end must have one entry per row of the band")
        if wmax is None:
            wmax = max(int(np.max(we - np.arange(r0, r1) - 1)) if n else 1, 1)
        wmax = int(wmax)
        w1 = max(wmax, 1)
        out_r2 = np.zeros((max(n, 1), w1), np.float64) if r2 else None
        out_cnt = np.zeros((max(n, 1), w1, 6), np.int32) if counts else None
        out_ab = np.zeros((max(n, 1), (w1 + 63) // 64), np.uint64) if threshold is not None else None
        self._chk(self._lib.gpca_ld_window(self._h, r0, r1, _vp(we), wmax, float(0.0 if threshold is None else threshold),
                                           _vp(out_r2), _vp(out_cnt), _vp(out_ab)))
        res = {}
        if r2:
            res["r2"] = out_r2[:n]
        if counts:
            res["counts"] = out_cnt[:n]
        if threshold is not None:
            res["above"] = out_ab[:n]
        return res

    def ld_score(self, win_end, wmax: Optional[int] = None, rows: Optional[Tuple[int, int]] = None, unbiased: bool = True,
                 partners: bool = False) -> dict:
        """LD scores of a band from the windowed-LD sweep (gpca_ld_score; gpca.h section a19), with ld_window's addressing: no pair
        leaves the device.  Returns {"score": int64 [span]} and, with partners=True, {"partners": int32 [span]}, span =
        min(K, row1 + wmax) - row0 entries from row0: the sum of rint(v 2^40) over the counted pairs of the band that hold the row (on
        either side), v = r2 - (1 - r2) / (n - 2) (unbiased) or r2, and the number of those pairs.  Exact integers, written per call:
        the caller adds its bands at their row0 (io.ld_score_sum)."""
        K = int(self._lib.gpca_num_pca_snps(self._h))
        r0, r1 = (0, K) if rows is None else (int(rows[0]), int(rows[1]))
        we = np.ascontiguousarray(win_end, np.int64)
        n = max(r1 - r0, 0)
        if we.shape != (n,):
            raise ValueError("win_end must have one entry per row of the band")
        if wmax is None:
            wmax = max(int(np.max(we - np.arange(r0, r1) - 1)) if n else 1, 1)
        wmax = int(wmax)
        span = max(min(K, r1 + max(wmax, 0)) - r0, 0) if n else 0
        score = np.zeros(max(span, 1), np.int64)
        part = np.zeros(max(span, 1), np.int32) if partners else None
        self._chk(self._lib.gpca_ld_score(self._h, r0, r1, _vp(we), wmax, _lib.LDSCORE_UNBIASED if unbiased else 0, _vp(score), _vp(part)))
        res = {"score": score[:span]}
        if partners:
            res["partners"] = part[:span]
        return res

    @staticmethod
    def ld_score_total(acc) -> np.ndarray:
        """L2 of every SNP (gpca_ld_score_total; host only): 1 + acc 2^-40 from the bands' scores added up (io.ld_score_sum); the 1 is
        the SNP with itself."""
        av = np.ascontiguousarray(acc, np.int64)
        if av.ndim != 1:
            raise ValueError("acc must be a vector of int64 sums")
        out = np.zeros(max(av.size, 1))
        lib = _lib.load()
        rc = lib.gpca_ld_score_total(_vp(av if av.size else np.zeros(1, np.int64)), av.size, _vp(out))
        if rc != 0:
            raise GpcaError(rc, "gpca_ld_score_total: " + lib.gpca_status_string(rc).decode())
        return out[:av.size]

    LDSC_FIELDS = ("m_used", "mean_chi2", "lambda_gc", "intercept", "intercept_se", "h2", "h2_se", "ratio", "ratio_se", "n_blocks")

    @staticmethod
    def ldsc_fit(chi2, ell, n_samples: float, M: float, w_ell=None, n_blocks: int = 200, chi2_max: Optional[float] = None) -> dict:
        """LD-score regression of chi2 on the LD scores ell (gpca_ldsc_fit; host only; the rule is written out in gpca.h section a19):
        iteratively reweighted least squares with a delete-one block jackknife.  Returns a dict of LDSC_FIELDS (m_used and n_blocks as
        int).  chi2_max None or 0: no cap."""
        cv = np.ascontiguousarray(chi2, np.float64)
        lv = np.ascontiguousarray(ell, np.float64)
        wv = None if w_ell is None else np.ascontiguousarray(w_ell, np.float64)
        if cv.ndim != 1 or lv.shape != cv.shape or (wv is not None and wv.shape != cv.shape):
            raise ValueError("chi2, ell and w_ell must be vectors of one length")
        out = np.zeros(10)
        one = np.zeros(1)
        lib = _lib.load()
        m = cv.size
        rc = lib.gpca_ldsc_fit(_vp(cv if m else one), _vp(lv if m else one), _vp(wv if (wv is None or m) else one), m, float(n_samples), float(M),
                               int(n_blocks), float(chi2_max or 0.0), _vp(out))
        if rc != 0:
            raise GpcaError(rc, "gpca_ldsc_fit: " + lib.gpca_status_string(rc).decode())
        res = dict(zip(GpcaEngine.LDSC_FIELDS, (float(v) for v in out)))
        res["m_used"], res["n_blocks"] = int(out[0]), int(out[9])
        return res

    def _pcr_args(self, pcs, train):
        N = self.dims()[1]
        V = np.ascontiguousarray(np.zeros((N, 0)) if pcs is None else pcs, np.float64)
        if V.ndim == 1:
            V = V.reshape(N, 1) if V.size == N else V.reshape(N, 0)
        if V.ndim != 2 or V.shape[0] != N:
            raise ValueError("pcs must be [N][P]: one row of coordinates per sample")
        t = None if train is None else np.ascontiguousarray(np.asarray(train) != 0, np.uint8)
        if t is not None and t.shape != (N,):
            raise ValueError("train must have one entry per sample")
        return N, V, t

    def pcrelate_isaf(self, pcs, train=None, rows: Optional[Tuple[int, int]] = None):
        """The regression of PC-Relate (gpca_pcrelate_isaf): kept rows [row0, row1) in PCA-SNP order (default: all) regressed on
        (1, pcs / rms) over the training samples (train: bool / uint8 [N], None = everyone).  Returns (mu [rows][N] f32: the
        individual-specific allele frequencies, beta [rows][P + 1] f32: the coefficients the device uses)."""
        N, V, t = self._pcr_args(pcs, train)
        K = int(self._lib.gpca_num_pca_snps(self._h))
        r0, r1 = (0, K) if rows is None else (int(rows[0]), int(rows[1]))
        n = max(r1 - r0, 0)
        mu = np.zeros((max(n, 1), N), np.float32)
        beta = np.zeros((max(n, 1), V.shape[1] + 1), np.float32)
        self._chk(self._lib.gpca_pcrelate_isaf(self._h, _vp(V), V.shape[1], _vp(t), r0, r1, _vp(mu), _vp(beta)))
        return mu[:n], beta[:n]

    def pcrelate(self, pcs, train=None, maf_bound: float = 0.01, rows: Optional[Tuple[int, int]] = None, nsnp: bool = False):
        """PC-Relate kinship of the kept rows (gpca_pcrelate): pcs [N][P] (P <= 32; None or P = 0: the homogeneous estimator), train as
        in pcrelate_isaf, maf_bound = tau: an entry counts when its call is observed and tau < mu < 1 - tau.  rows = (row0, row1): rows
        [row0, row1) of the lower triangle WITH the diagonal packed row-major (element (a, b <= a) at a (a + 1) / 2 - row0 (row0 + 1) / 2
        + b), f64; rows = None: the full symmetric [N][N] f64 array.  The diagonal is the self-kinship (1 + F) / 2; NaN where a pair
        shares no valid SNP.  nsnp=True also returns the int32 count of SNPs valid in both samples, in the same shape."""
        N, V, t = self._pcr_args(pcs, train)
        r0, r1 = (0, N) if rows is None else (int(rows[0]), int(rows[1]))
        E = _band_entries(r0, r1, True)
        k = np.empty(max(E, 1), np.float64)
        cnt = np.empty(max(E, 1), np.int32) if nsnp else None
        self._chk(self._lib.gpca_pcrelate(self._h, _vp(V), V.shape[1], _vp(t), float(maf_bound), r0, r1, _vp(k), _vp(cnt)))
        k = k[:E]
        cnt = cnt[:E] if nsnp else None
        if rows is not None:
            return (k, cnt) if nsnp else k
        full = _band_to_full(k, N, True)
        return (full, _band_to_full(cnt, N, True)) if nsnp else full

    @staticmethod
    def _assoc_design(covar, include, N):
        """(Cv [N][Pc] f64, inc uint8 [N] or None) of an association call, checked."""
        Cv = np.ascontiguousarray(np.zeros((N, 0)) if covar is None else covar, np.float64)
        if Cv.ndim == 1:
            Cv = Cv.reshape(N, 0) if Cv.size == 0 else Cv.reshape(-1, 1)
        if Cv.ndim != 2 or Cv.shape[0] != N:
            raise ValueError("covar must be [N][Pc]: one row of covariates per sample")
        inc = None if include is None else np.ascontiguousarray(np.asarray(include) != 0, np.uint8)
        if inc is not None and inc.shape != (N,):
            raise ValueError("include must have one entry per sample")
        return Cv, inc

    def _assoc_args(self, Y, covar, include, rows):
        """(Yv, Cv, inc, T, Pc, r0, r1, n) of an association scan: the checked arrays, their widths, the band and its row count."""
        N = self.dims()[1]
        Yv = np.ascontiguousarray(Y, np.float64)
        if Yv.ndim == 1:
            Yv = Yv.reshape(-1, 1)
        if Yv.ndim != 2 or Yv.shape[0] != N:
            raise ValueError("Y must be [N][T]: one row of traits per sample")
        Cv, inc = self._assoc_design(covar, include, N)
        T, Pc = Yv.shape[1], Cv.shape[1]
        K = int(self._lib.gpca_num_pca_snps(self._h))
        r0, r1 = (0, K) if rows is None else (int(rows[0]), int(rows[1]))
        return Yv, Cv, inc, T, Pc, r0, r1, max(r1 - r0, 0)

    def assoc_linear(self, Y, covar=None, include=None, max_vif: float = 50.0, rows: Optional[Tuple[int, int]] = None, xb: bool = False):
        """Linear association scan (gpca_assoc_linear): ordinary least squares of every trait (column of Y [N][T]) on (1, covar, g)
        for the kept rows [row0, row1) in PCA-SNP order (default: all); covar [N][Pc] or None, T + Pc <= 64; include: bool / uint8 [N],
        None = everyone.  A missing call is imputed to the row's mean over the included samples.  Returns a dict: beta, se, t
        [rows][T]; n_obs, a1_freq, xx, sxx [rows]; with xb=True also xb [rows][T + Pc] (the products the statistics come from).
        beta, se and t are NaN for a row with no observed call, no variance, a variance inflation above max_vif, or rss <= 0."""
        Yv, Cv, inc, T, Pc, r0, r1, n = self._assoc_args(Y, covar, include, rows)
        stats = np.zeros((max(n, 1), max(T, 1), 3), np.float64)
        info = np.zeros((max(n, 1), 4), np.float64)
        out_xb = np.zeros((max(n, 1), max(T + Pc, 1)), np.float64) if xb else None
        self._chk(self._lib.gpca_assoc_linear(self._h, _vp(Yv), T, _vp(Cv) if Pc else None, Pc, _vp(inc), float(max_vif), r0, r1,
                                              _vp(stats), _vp(out_xb), _vp(info)))
        res = {"beta": stats[:n, :, 0], "se": stats[:n, :, 1], "t": stats[:n, :, 2], "n_obs": info[:n, 0], "a1_freq": info[:n, 1],
               "xx": info[:n, 2], "sxx": info[:n, 3]}
        if xb:
            res["xb"] = out_xb[:n]
        return res

    @staticmethod
    def student_t_log10p(t: float, df: float) -> float:
        """-log10 of the two-sided p-value of a Student t statistic (gpca_student_t_log10p; host only, no underflow)."""
        return float(_lib.load().gpca_student_t_log10p(float(t), float(df)))

    def assoc_qtl(self, Y, covar=None, include=None, max_vif: float = 50.0, r2_min: Optional[float] = None, t_min: Optional[float] = None,
                  cap: Optional[int] = None, rows: Optional[Tuple[int, int]] = None, best: bool = True):
        """Many-trait QTL scan (gpca_assoc_qtl; gpca.h section a24): assoc_linear's regression of the kept rows [row0, row1) (default:
        all) against every column of Y [N][T], T up to 2^20, of which the pairs with r2 >= r2_min come back, and the best row of every
        trait.  Exactly one of r2_min (in [0, 1]) and t_min (a cutoff on |t|, turned once into r2_min = t^2 / (t^2 + df)) is given.
        cap: the record buffer; None = sized by a first call, filled by a second.  Returns a dict: n_obs, a1_freq, xx, sxx [rows]; yy
        [T]; df; r2_min; hit_count uint32 [rows]; n_found; rows (absolute kept rows, uint32), traits (uint32), xb, r2 [n_found] in
        ascending (row, trait) order, or None each when n_found > cap; with best=True best_r2 [T] and best_row int64 [T] (NaN and -1
        for a trait without a live row).  xb of a hit is assoc_linear's, bit for bit; qtl_stats turns it into beta, se, t."""
        Yv, Cv, inc, T, Pc, r0, r1, n = self._assoc_args(Y, covar, include, rows)
        if (r2_min is None) == (t_min is None):
            raise ValueError("exactly one of r2_min and t_min must be given")
        N = self.dims()[1]
        df = float((N if inc is None else int(inc.sum())) - Pc - 2)
        if t_min is not None:
            t2 = float(t_min) * float(t_min)
            r2_min = t2 / (t2 + df)
        info = np.zeros((max(n, 1), 4), np.float64)
        yy = np.zeros(max(T, 1), np.float64)
        hit_count = np.zeros(max(n, 1), np.uint32)
        b2 = np.zeros(max(T, 1), np.float64) if best else None
        bw = np.zeros(max(T, 1), np.int64) if best else None
        found = C.c_int64(0)
        size = 0 if cap is None else int(cap)
        while True:
            hi = np.zeros((max(size, 1), 2), np.uint32)
            hv = np.zeros((max(size, 1), 2), np.float64)
            self._chk(self._lib.gpca_assoc_qtl(self._h, _vp(Yv), T, _vp(Cv) if Pc else None, Pc, _vp(inc), float(max_vif), float(r2_min), r0, r1,
                                               _vp(info), _vp(yy), _vp(hit_count), _vp(hi) if size > 0 else None, _vp(hv) if size > 0 else None,
                                               size, C.byref(found), _vp(b2), _vp(bw)))
            nf = int(found.value)
            if nf <= size or cap is not None:
                break
            size = nf
        res = {"n_obs": info[:n, 0], "a1_freq": info[:n, 1], "xx": info[:n, 2], "sxx": info[:n, 3], "yy": yy[:T], "df": df,
               "r2_min": float(r2_min), "hit_count": hit_count[:n], "n_found": nf}
        ok = nf <= size
        res["rows"] = hi[:nf, 0].copy() if ok else None
        res["traits"] = hi[:nf, 1].copy() if ok else None
        res["xb"] = hv[:nf, 0].copy() if ok else None
        res["r2"] = hv[:nf, 1].copy() if ok else None
        if best:
            res["best_r2"], res["best_row"] = b2[:T], bw[:T]
        return res

    @staticmethod
    def qtl_t_min(log10p: float, df: float) -> float:
        """The |t| cutoff of a threshold on -log10 p at df degrees of freedom (gpca_qtl_t_min: bisection on student_t_log10p)."""
        return float(_lib.load().gpca_qtl_t_min(float(log10p), float(df)))

    @staticmethod
    def qtl_stats(xb, sxx, yy, df: float) -> np.ndarray:
        """The host rule on the hits of assoc_qtl (gpca_qtl_stats): [n][3] = beta, se, t of the pairs with products xb, row sums sxx and
        trait sums yy (arrays of one length, or scalars), by assoc_linear's formulas; NaN where rss <= 0."""
        lib = _lib.load()
        xv, sv, yv = np.broadcast_arrays(np.asarray(xb, np.float64), np.asarray(sxx, np.float64), np.asarray(yy, np.float64))
        out = np.zeros((xv.size, 3), np.float64)
        tmp = (C.c_double * 3)()
        for i, (a, b, c) in enumerate(zip(xv.ravel(), sv.ravel(), yv.ravel())):
            lib.gpca_qtl_stats(float(a), float(b), float(c), float(df), tmp)
            out[i] = tmp[0], tmp[1], tmp[2]
        return out

    def assoc_qtl_cis(self, Y, win, covar=None, include=None, max_vif: float = 50.0, perm=None, n_perm: int = 0, seed: int = 0):
        """cis-QTL mapping (gpca_assoc_qtl_cis; gpca.h section a25): for every column of Y [N][G] the best kept row of its own window
        win [G][2] = [lo, hi) and the best r2 of P permutations of the trait over the same window.  perm: uint32 [P][n], every row a
        permutation of the n included samples; None with n_perm > 0: qtl_perm_table(seed, n, n_perm).  Returns a dict: n_var int64 [G],
        best_row int64 [G], best_r2 [G], best_stat [G][3] = xb, sxx, yy (qtl_stats applies), perm_r2 [G][P], df, perm (the table used).  A
        window without a live row gives n_var = 0, best_row = -1 and NaN elsewhere."""
        Yv, Cv, inc, G, Pc, _, _, _ = self._assoc_args(Y, covar, include, None)
        N = self.dims()[1]
        n = N if inc is None else int(np.count_nonzero(inc))
        wv = np.ascontiguousarray(win, np.int64)
        if wv.shape != (G, 2):
            raise ValueError("win must be [G][2]: a range [lo, hi) of kept rows per trait")
        if perm is None:
            perm = GpcaEngine.qtl_perm_table(seed, n, int(n_perm)) if n_perm else np.zeros((0, n), np.uint32)
        pv = np.ascontiguousarray(perm, np.uint32)
        if pv.ndim != 2 or pv.shape[1] != n:
            raise ValueError("perm must be [P][n]: one permutation of the n included samples per row")
        P = pv.shape[0]
        n_var, best_row = np.zeros(max(G, 1), np.int64), np.zeros(max(G, 1), np.int64)
        best_r2, best_stat = np.zeros(max(G, 1), np.float64), np.zeros((max(G, 1), 3), np.float64)
        perm_r2 = np.zeros((max(G, 1), max(P, 1)), np.float64)
        self._chk(self._lib.gpca_assoc_qtl_cis(self._h, _vp(Yv), G, _vp(Cv) if Pc else None, Pc, _vp(inc), float(max_vif), _vp(wv),
                                               _vp(pv) if P else None, P, _vp(n_var), _vp(best_row), _vp(best_r2), _vp(best_stat),
                                               _vp(perm_r2) if P else None))
        return {"n_var": n_var[:G], "best_row": best_row[:G], "best_r2": best_r2[:G], "best_stat": best_stat[:G], "perm_r2": perm_r2[:G, :P],
                "df": float(n - Pc - 2), "perm": pv}

    def qtl_perm_panel(self, b, Q, perm) -> np.ndarray:
        """The permuted columns of a25's panel (gpca_qtl_perm_panel) for the residual b [n], the basis Q [n][Pc] (None or [n][0]: no
        covariates) and the table perm uint32 [P][n]: float32 [P][n]."""
        bv = np.ascontiguousarray(b, np.float64).reshape(-1)
        n = bv.shape[0]
        Qv = np.zeros((n, 0), np.float64) if Q is None else np.ascontiguousarray(Q, np.float64).reshape(n, -1)
        pv = np.ascontiguousarray(perm, np.uint32)
        if pv.ndim != 2 or pv.shape[1] != n:
            raise ValueError("perm must be [P][n]")
        P, Pc = pv.shape[0], Qv.shape[1]
        out = np.zeros((max(P, 1), max(n, 1)), np.float32)
        self._chk(self._lib.gpca_qtl_perm_panel(self._h, _vp(bv), _vp(Qv) if Pc else None, Pc, n, _vp(pv) if P else None, P, _vp(out)))
        return out[:P, :n]

    @staticmethod
    def qtl_perm_table(seed: int, n: int, P: int) -> np.ndarray:
        """The permutation table of a25 (gpca_qtl_perm_table; host only): uint32 [P][n], row p a Fisher-Yates shuffle of 0 .. n - 1 driven
        by philox4x32-10 keyed by (seed, p)."""
        out = np.zeros((max(int(P), 0), max(int(n), 0)), np.uint32)
        rc = _lib.load().gpca_qtl_perm_table(int(seed) & 0xFFFFFFFFFFFFFFFF, int(n), int(P), _vp(out) if out.size else None)
        if rc != 0:
            raise GpcaError(rc, "gpca_qtl_perm_table: n >= 0 and 0 <= P <= 65535 are required")
        return out

    @staticmethod
    def qtl_beta_approx(perm_r2, r2_nominal: float, df: float) -> dict:
        """FastQTL's beta approximation of the permutation p-value (gpca_qtl_beta_approx; host only): a dict of pval_perm, true_df,
        shape1, shape2, log10p_nominal_true, log10p_beta, shape1_mom and status (bit 1: no root for true_df, df used; bit 2: the
        maximum-likelihood fit failed, moment estimates returned)."""
        pv = np.ascontiguousarray(perm_r2, np.float64).reshape(-1)
        out = np.zeros(7, np.float64)
        st = C.c_int32(0)
        rc = _lib.load().gpca_qtl_beta_approx(_vp(pv) if pv.size else None, pv.size, float(r2_nominal), float(df), _vp(out), C.byref(st))
        if rc != 0:
            raise GpcaError(rc, "gpca_qtl_beta_approx: bad argument")
        keys = ("pval_perm", "true_df", "shape1", "shape2", "log10p_nominal_true", "log10p_beta", "shape1_mom")
        res = {k: float(v) for k, v in zip(keys, out)}
        res["status"] = int(st.value)
        return res

    def assoc_logistic_score(self, Y, covar=None, include=None, max_vif: float = 50.0, rows: Optional[Tuple[int, int]] = None, ua: bool = False):
        """Logistic score scan (gpca_assoc_logistic_score): the score test of every case / control trait (column of Y [N][T], 0 / 1 on
        the included samples) for the kept rows [row0, row1) in PCA-SNP order (default: all), the null model logit P(y = 1) = (1, covar)
        alpha fitted once per trait; covar [N][Pc] or None, T (Pc + 3) <= 64; include: bool / uint8 [N], None = everyone.  A missing
        call is imputed to the row's mean over the included samples.  Returns a dict: beta, se, z, vw, V [rows][T]; n_obs, a1_freq, xx,
        flipped [rows]; with ua=True also ua [rows][T][Pc + 3] = U, gwg, a_0 .. a_Pc in the operand's coding (2 - g on a flipped row).
        beta, se and z (for allele A1) are NaN for a row with no observed call, no variance, V <= 0 or a variance inflation above
        max_vif."""
        return self._assoc_logistic(Y, covar, include, max_vif, None, rows, ua)

    def assoc_logistic_spa(self, Y, covar=None, include=None, max_vif: float = 50.0, spa_z: float = 2.0,
                           rows: Optional[Tuple[int, int]] = None, ua: bool = False):
        """Logistic score scan with the saddle-point correction (gpca_assoc_logistic_spa): assoc_logistic_score's arguments and its
        dict with the same bits, and beside them log10p, spa_status, zeta [rows][T] (and zeta [rows][T][2]).  Where |z| >= spa_z
        (at least 0.5, or inf for no correction; SAIGE's 2 by default) the two-sided -log10 p comes from the saddle-point approximation
        of U's distribution under the null (spa_status 1; 2 where a tail did not converge: the normal value); elsewhere it is the
        normal value of z (spa_status 0).  zeta are the two tails' roots in the operand's coding; NaN statistics give NaN."""
        return self._assoc_logistic(Y, covar, include, max_vif, float(spa_z), rows, ua)

    def assoc_logistic_firth(self, Y, covar=None, include=None, max_vif: float = 50.0, firth_z: float = 1.959964,
                             rows: Optional[Tuple[int, int]] = None, ua: bool = False):
        """Logistic score scan with the approximate Firth correction (gpca_assoc_logistic_firth): assoc_logistic_score's arguments and
        its dict with the same bits, and beside them log10p, firth_status, firth_beta, firth_se, firth_lrt [rows][T].  Where
        |z| >= firth_z (at least 0, or inf for no correction; two-sided 0.05 by default) one coefficient on the covariate-adjusted
        genotype is fitted by Firth's penalised likelihood with the null model as offset: -log10 p is the chi^2_1 value of the penalised
        likelihood-ratio statistic firth_lrt, firth_beta (for allele A1) and firth_se = 1 / sqrt(information) are finite under
        separation (firth_status 1; 2 where the root rule failed: the normal value); elsewhere -log10 p is the normal value of z and
        the rest NaN (firth_status 0)."""
        return self._assoc_logistic(Y, covar, include, max_vif, None, rows, ua, firth_z=float(firth_z))

    def _assoc_logistic(self, Y, covar, include, max_vif, spa_z, rows, ua, firth_z=None):
        Yv, Cv, inc, T, Pc, r0, r1, n = self._assoc_args(Y, covar, include, rows)
        stats = np.zeros((max(n, 1), max(T, 1), 5), np.float64)
        info = np.zeros((max(n, 1), 5), np.float64)
        out_ua = np.zeros((max(n, 1), max(T, 1), Pc + 3), np.float64) if ua else None
        if firth_z is not None:
            firth = np.zeros((max(n, 1), max(T, 1), 5), np.float64)
            self._chk(self._lib.gpca_assoc_logistic_firth(self._h, _vp(Yv), T, _vp(Cv) if Pc else None, Pc, _vp(inc), float(max_vif), firth_z,
                                                          r0, r1, _vp(stats), _vp(firth), _vp(out_ua), _vp(info)))
        elif spa_z is None:
            self._chk(self._lib.gpca_assoc_logistic_score(self._h, _vp(Yv), T, _vp(Cv) if Pc else None, Pc, _vp(inc), float(max_vif), r0, r1,
                                                          _vp(stats), _vp(out_ua), _vp(info)))
        else:
            spa = np.zeros((max(n, 1), max(T, 1), 4), np.float64)
            self._chk(self._lib.gpca_assoc_logistic_spa(self._h, _vp(Yv), T, _vp(Cv) if Pc else None, Pc, _vp(inc), float(max_vif), spa_z, r0,
                                                        r1, _vp(stats), _vp(spa), _vp(out_ua), _vp(info)))
        res = {"beta": stats[:n, :, 0], "se": stats[:n, :, 1], "z": stats[:n, :, 2], "vw": stats[:n, :, 3], "V": stats[:n, :, 4],
               "n_obs": info[:n, 0], "a1_freq": info[:n, 1], "xx": info[:n, 2], "flipped": info[:n, 3]}
        if ua:
            res["ua"] = out_ua[:n]
        if firth_z is not None:
            res.update(log10p=firth[:n, :, 0], firth_status=firth[:n, :, 1], firth_beta=firth[:n, :, 2], firth_se=firth[:n, :, 3],
                       firth_lrt=firth[:n, :, 4])
        elif spa_z is not None:
            res.update(log10p=spa[:n, :, 0], spa_status=spa[:n, :, 1], zeta=spa[:n, :, 2:4])
        return res

    def assoc_logistic_set(self, Y, sets, covar=None, include=None, max_vif: float = 50.0, ua: bool = False):
        """Gene-level set scan (gpca_assoc_logistic_set; gpca.h section a16): sets = a sequence of sets, each 1 .. 128 strictly ascending
        kept rows in PCA-SNP order; the other arguments are assoc_logistic_score's.  Returns assoc_logistic_score's dict over the LISTED
        rows (the sets' rows one set after the other, with the bits the score scan gives each row), "set_off" [n_sets + 1] = where each
        set starts in that list, and "phi" = per set the covariance of its scores for allele A1, [T][m][m] symmetric.  Feed
        u = sign * U (sign = -1 on a flipped row; with ua=True, U = ua[..., 0]) and phi[s][t] to set_test."""
        Yv, Cv, inc, T, Pc, _, _, _ = self._assoc_args(Y, covar, include, None)
        sets = [np.ascontiguousarray(s, np.int64).reshape(-1) for s in sets]
        off = np.zeros(len(sets) + 1, np.int64)
        if sets:
            off[1:] = np.cumsum([s.shape[0] for s in sets])
        rows = np.ascontiguousarray(np.concatenate(sets) if sets else np.zeros(0, np.int64), np.int64)
        n = int(off[-1])
        tri = [int(s.shape[0]) * (int(s.shape[0]) + 1) // 2 for s in sets]
        stats = np.zeros((max(n, 1), max(T, 1), 5), np.float64)
        info = np.zeros((max(n, 1), 5), np.float64)
        out_ua = np.zeros((max(n, 1), max(T, 1), Pc + 3), np.float64) if ua else None
        phi = np.zeros(max(sum(tri) * max(T, 1), 1), np.float64)
        self._chk(self._lib.gpca_assoc_logistic_set(self._h, _vp(Yv), T, _vp(Cv) if Pc else None, Pc, _vp(inc), float(max_vif), len(sets),
                                                    _vp(off), _vp(rows), _vp(stats), _vp(out_ua), _vp(info), _vp(phi)))
        res = {"beta": stats[:n, :, 0], "se": stats[:n, :, 1], "z": stats[:n, :, 2], "vw": stats[:n, :, 3], "V": stats[:n, :, 4],
               "n_obs": info[:n, 0], "a1_freq": info[:n, 1], "xx": info[:n, 2], "flipped": info[:n, 3], "set_off": off}
        if ua:
            res["ua"] = out_ua[:n]
        full, p0 = [], 0
        for s, nt in zip(sets, tri):
            m = int(s.shape[0])
            il = np.tril_indices(m)
            f = np.zeros((T, m, m), np.float64)
            for t in range(T):
                lo = phi[p0 + t * nt: p0 + (t + 1) * nt]
                f[t][il] = lo
                f[t].T[il] = lo
            full.append(f)
            p0 += T * nt
        res["phi"] = full
        return res

    @staticmethod
    def set_test(u, phi, weight=None):
        """The burden and SKAT tests of one set (gpca_set_test; host only; gpca.h section a16): u [m] = the scores for allele A1,
        phi [m][m] = their covariance (the lower triangle is read), weight [m] or None = 1.  Returns a dict: m_used, burden_beta,
        burden_se, burden_z, burden_log10p, skat_q, skat_log10p, skat_status (0 the bulk value, 1 the saddle point, 2 the bulk value
        after a failed saddle point), z_q, zeta."""
        uv = np.ascontiguousarray(u, np.float64).reshape(-1)
        m = uv.shape[0]
        pv = np.asarray(phi, np.float64)
        if pv.shape != (m, m):
            raise ValueError("phi must be [m][m] for u [m]")
        lo = np.ascontiguousarray(pv[np.tril_indices(m)])
        wv = None if weight is None else np.ascontiguousarray(weight, np.float64).reshape(-1)
        if wv is not None and wv.shape[0] != m:
            raise ValueError("weight must have one entry per row")
        out = np.zeros(10)
        lib = _lib.load()
        rc = lib.gpca_set_test(_vp(uv), _vp(lo), _vp(wv), m, _vp(out))
        if rc != 0:
            raise GpcaError(rc, "gpca_set_test: " + lib.gpca_status_string(rc).decode())
        keys = ("m_used", "burden_beta", "burden_se", "burden_z", "burden_log10p", "skat_q", "skat_log10p", "skat_status", "z_q", "zeta")
        res = {k: float(v) for k, v in zip(keys, out)}
        res["m_used"], res["skat_status"] = int(out[0]), int(out[7])
        return res

    def group_counts(self, group, n_groups: Optional[int] = None, rows: Optional[Tuple[int, int]] = None) -> np.ndarray:
        """Genotype counts inside sample groups (gpca_group_counts; gpca.h section a17): group [N] = every sample's group 0 .. P - 1, or
        -1 for none; n_groups = P (default: the largest label + 1, at least 1; at most 64); rows = (row0, row1): the kept rows
        [row0, row1) in PCA-SNP order (default: all).  Returns uint32 [rows][P][3] = n_obs, n_het, n_hom2: the group's samples with an
        observed call on the row, with g = 1 and with g = 2 (copies of A1).  Exact integers; a band carries the bits of the full call."""
        N = self.dims()[1]
        gv = np.asarray(group)
        if gv.shape != (N,) or gv.dtype.kind not in "iu":
            raise ValueError("group must be an integer array with one label per sample")
        gv = np.ascontiguousarray(np.clip(gv.astype(np.int64), -1, 1 << 30), np.int32)
        P = int(n_groups) if n_groups is not None else max(int(gv.max(initial=-1)) + 1, 1)
        K = int(self._lib.gpca_num_pca_snps(self._h))
        r0, r1 = (0, K) if rows is None else (int(rows[0]), int(rows[1]))
        n = max(r1 - r0, 0)
        out = np.zeros((max(n, 1), max(min(P, 64), 1), 3), np.uint32)
        self._chk(self._lib.gpca_group_counts(self._h, _vp(gv), P, r0, r1, _vp(out)))
        return out[:n]

    def f2_blocks(self, group, block, n_groups: Optional[int] = None, n_blocks: Optional[int] = None,
                  rows: Optional[Tuple[int, int]] = None, counts: bool = False):
        """f2 jackknife blocks (gpca_f2_blocks; gpca.h section a23): group and rows as in group_counts (n_groups = P, 2 .. 64); block =
        one jackknife block id per row of the band, 0 .. B - 1, or -1 for a row that enters nothing; n_blocks = B (default: the largest
        id + 1, at least 1).  Returns (acc, cnt), both int64 [B][P (P - 1) / 2]: per block and pair (i, j), j < i, at i (i - 1) / 2 + j,
        the sum of rint(f2 2^40) over the block's rows on which both groups have a call, and the number of those rows; with counts=True
        also group_counts' uint32 [rows][P][3] of the band, from the same genotype pass.  Exact integers, written per call: the caller
        adds its bands."""
        N = self.dims()[1]
        gv = np.asarray(group)
        if gv.shape != (N,) or gv.dtype.kind not in "iu":
            raise ValueError("group must be an integer array with one label per sample")
        gv = np.ascontiguousarray(np.clip(gv.astype(np.int64), -1, 1 << 30), np.int32)
        P = int(n_groups) if n_groups is not None else max(int(gv.max(initial=-1)) + 1, 1)
        K = int(self._lib.gpca_num_pca_snps(self._h))
        r0, r1 = (0, K) if rows is None else (int(rows[0]), int(rows[1]))
        n = max(r1 - r0, 0)
        bv = np.asarray(block)
        if bv.shape != (n,) or bv.dtype.kind not in "iu":
            raise ValueError("block must be an integer array with one block id per row of the band")
        bq = np.zeros(max(n, 1), np.int32)
        bq[:n] = np.clip(bv.astype(np.int64), -(1 << 30), 1 << 30)
        B = int(n_blocks) if n_blocks is not None else max(int(bv.max(initial=-1)) + 1, 1)
        Pc = max(min(P, 64), 2)
        pairs = Pc * (Pc - 1) // 2
        acc = np.zeros((max(B, 1), pairs), np.int64)
        cnt = np.zeros((max(B, 1), pairs), np.int64)
        cv = np.zeros((max(n, 1), Pc, 3), np.uint32) if counts else None
        self._chk(self._lib.gpca_f2_blocks(self._h, _vp(gv), P, r0, r1, _vp(bq), B, _vp(acc), _vp(cnt), _vp(cv)))
        return (acc, cnt, cv[:n]) if counts else (acc, cnt)

    @staticmethod
    def fstat(acc, cnt, quads) -> np.ndarray:
        """f2, f3 and f4 with their weighted block-jackknife standard errors (gpca_fstat; gpca.h section a23; host only).  acc and cnt
        [B][pairs] = the bands of f2_blocks added up; quads [M][4] = (a, b, c, d) per statistic, read as f4(a, b; c, d), so that
        f2(A, B) = (A, B, A, B) and f3(C; A, B) = (C, A, C, B).  Returns float64 [M][6] = theta, the jackknife estimate, se, z = theta /
        se, the blocks used, the fewest SNPs behind one of its pairs."""
        av, cv = np.ascontiguousarray(acc, np.int64), np.ascontiguousarray(cnt, np.int64)
        if av.ndim != 2 or av.shape != cv.shape:
            raise ValueError("acc and cnt must be [B][pairs] as f2_blocks returns them")
        B, pairs = av.shape
        P = int(round((1.0 + np.sqrt(1.0 + 8.0 * pairs)) / 2.0))
        if P * (P - 1) // 2 != pairs:
            raise ValueError(f"{pairs} is not a number of pairs P (P - 1) / 2")
        qv = np.ascontiguousarray(quads, np.int32).reshape(-1, 4)
        M = qv.shape[0]
        out = np.zeros((max(M, 1), 6), np.float64)
        lib = _lib.load()
        rc = lib.gpca_fstat(_vp(av), _vp(cv), B, P, _vp(qv if M else np.zeros((1, 4), np.int32)), M, _vp(out))
        if rc != _lib.GPCA_OK:
            raise GpcaError(rc, "gpca_fstat: " + lib.gpca_status_string(rc).decode())
        return out[:M]

    def sample_counts(self, weights=None, rows: Optional[Tuple[int, int]] = None) -> dict:
        """Genotype counts per sample (gpca_sample_counts; gpca.h section a18) over the kept rows [row0, row1) in PCA-SNP order
        (rows; default: all).  Returns {"counts": uint32 [N][3] = n_obs, n_het, n_hom2 (the rows on which the sample has an observed
        call, g = 1 and g = 2), "qsum": uint64 [N] = the sum of weights[j] over the rows on which the sample is observed, or None
        without weights}.  weights: uint32, one per row of the band, each at most 2^30 (het_weights).  Exact integers, written per
        call: the caller sums its bands."""
        N = self.dims()[1]
        K = int(self._lib.gpca_num_pca_snps(self._h))
        r0, r1 = (0, K) if rows is None else (int(rows[0]), int(rows[1]))
        n = max(r1 - r0, 0)
        qv = None
        if weights is not None:
            wv = np.asarray(weights)
            if wv.shape != (n,) or wv.dtype.kind not in "iu" or (wv.size and (int(wv.min()) < 0 or int(wv.max()) > 0xffffffff)):
                raise ValueError("weights must be an unsigned integer array with one entry per row of the band")
            qv = np.zeros(max(n, 1), np.uint32)
            qv[:n] = wv
        counts = np.zeros((max(N, 1), 3), np.uint32)
        qsum = None if qv is None else np.zeros(max(N, 1), np.uint64)
        self._chk(self._lib.gpca_sample_counts(self._h, r0, r1, _vp(qv), _vp(counts), _vp(qsum)))
        return {"counts": counts[:N], "qsum": None if qsum is None else qsum[:N]}

    def _admix_shape(self, K) -> Tuple[int, int, int]:
        return self.dims()[1], int(self._lib.gpca_num_pca_snps(self._h)), int(K)

    @staticmethod
    def _admix_mode(mode, N):
        if mode is None:
            return None
        mv = np.ascontiguousarray(mode, np.uint8)
        if mv.shape != (N,):
            raise ValueError("mode must hold one byte per sample (0 = free, 1 = Q fixed, 2 = projected)")
        return mv

    def admix_init(self, K: int, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """The starting point of the admixture fit (gpca_admix_init; gpca.h section a21): (Q float32 [N][K], F float32 [Kr][K]) over
        the kept rows, a pure function of (seed, K, N, Kr, the kept rows' observed A1 frequencies)."""
        N, Kr, K = self._admix_shape(K)
        Q = np.zeros((max(N, 1), max(K, 1)), np.float32)
        F = np.zeros((max(Kr, 1), max(K, 1)), np.float32)
        self._chk(self._lib.gpca_admix_init(self._h, K, int(seed) & 0xffffffffffffffff, _vp(Q), _vp(F)))
        return Q[:N], F[:Kr]

    def admix_step(self, Q, F, mode=None) -> Tuple[np.ndarray, np.ndarray, float]:
        """One EM step of the admixture model (gpca_admix_step; gpca.h section a21) from Q [N][K] and F [Kr][K] exactly as given:
        (Q', F', loglik of (Q, F)).  mode: one byte per sample, 0 = Q free and the sample contributes to F, 1 = Q stays and the sample
        contributes, 2 = Q free and the sample does not contribute."""
        Qv, Fv = np.ascontiguousarray(Q, np.float32), np.ascontiguousarray(F, np.float32)
        if Qv.ndim != 2 or Fv.ndim != 2 or Qv.shape[1] != Fv.shape[1]:
            raise ValueError("Q must be [N][K] and F [Kr][K]")
        N, Kr, K = self._admix_shape(Qv.shape[1])
        if Kr > 0 and (Qv.shape != (N, K) or Fv.shape != (Kr, K)):       # (no kept row: the library says what is missing)
            raise ValueError(f"Q must be [{N}][K] and F [{Kr}][K] (the samples and the kept rows of the handle)")
        mv = self._admix_mode(mode, N)
        Qn, Fn, ll = np.zeros_like(Qv), np.zeros_like(Fv), C.c_double()
        self._chk(self._lib.gpca_admix_step(self._h, K, _vp(Qv), _vp(Fv), _vp(mv), _vp(Qn), _vp(Fn), C.byref(ll)))
        return Qn, Fn, ll.value

    def admix(self, K: int, seed: int = 0, max_iter: int = 2000, tol: float = 1e-7, accel: bool = True, mode=None, Q=None, F=None) -> dict:
        """Admixture proportions (gpca_admix; gpca.h section a21): the ADMIXTURE model with K ancestries fitted by EM, with SQUAREM
        acceleration unless accel is False, over the kept rows and all samples.  Starts from admix_init(K, seed), or from Q and F when
        both are given.  Returns {"Q": float32 [N][K], "F": float32 [Kr][K], "loglik", "steps", "cycles", "converged", "fallbacks",
        "trace": the cycle-start log-likelihoods (the first 2^20 at most)}.  max_iter counts EM steps; reaching it is not an error (converged is False)."""
        if (Q is None) != (F is None):
            raise ValueError("Q and F go together (both or neither)")
        N, Kr, K = self._admix_shape(K)
        if Q is None:
            Qv, Fv = np.zeros((max(N, 1), max(K, 1)), np.float32), np.zeros((max(Kr, 1), max(K, 1)), np.float32)
        else:
            Qv, Fv = np.array(Q, np.float32, order="C"), np.array(F, np.float32, order="C")
            if Kr > 0 and (Qv.shape != (N, K) or Fv.shape != (Kr, K)):
                raise ValueError(f"Q must be [{N}][{K}] and F [{Kr}][{K}]")
        mv = self._admix_mode(mode, N)
        trace = np.zeros(min(max(int(max_iter), 1), 1 << 20), np.float64)           # (a cycle is at least one step; 2^20 cycles at most are kept)
        par = _lib.gpca_admix_params(K, int(max_iter), int(seed) & 0xffffffffffffffff, float(tol), 1 if accel else 0, 0 if Q is None else 1)
        info = _lib.gpca_admix_info()
        info.trace, info.trace_cap = trace.ctypes.data, trace.size
        self._chk(self._lib.gpca_admix(self._h, C.byref(par), _vp(mv), _vp(Qv), _vp(Fv), C.byref(info)))
        return {"Q": Qv[:N], "F": Fv[:Kr], "loglik": info.loglik, "steps": int(info.steps), "cycles": int(info.cycles),
                "converged": bool(info.converged), "fallbacks": int(info.fallbacks), "trace": trace[:min(int(info.cycles), trace.size)].copy()}

    @staticmethod
    def admix_cv_fold(seed: int, folds: int, rows: int, N: int, row0: int = 0) -> np.ndarray:
        """The fold of every call of the admixture cross-validation (gpca_admix_cv_fold; host only; gpca.h section a22): uint8
        [rows][N] for the kept rows row0 .. row0 + rows - 1 (positions among the kept rows, PCA-SNP order) and the samples 0 .. N - 1."""
        out = np.zeros((max(int(rows), 1), max(int(N), 1)), np.uint8)
        lib = _lib.load()
        rc = lib.gpca_admix_cv_fold(int(seed) & 0xffffffffffffffff, int(folds), int(row0), int(rows), int(N), _vp(out))
        if rc != 0:
            raise GpcaError(rc, "gpca_admix_cv_fold: folds must be 2 .. 64 and the extents non-negative: " + lib.gpca_status_string(rc).decode())
        return out[:max(int(rows), 0), :max(int(N), 0)]

    def admix_step_holdout(self, Q, F, folds: int, fold: int, cv_seed: int = 0, mode=None) -> dict:
        """One hold-out step of the admixture model (gpca_admix_step_holdout; gpca.h section a22): admix_step with the observed calls of
        fold `fold` (of `folds`, under cv_seed) counted as missing.  Returns {"Q", "F", "loglik"} of that step and, evaluated at the
        input Q and F over the held-out calls, {"held_loglik", "n_held", "n_het_held"}."""
        Qv, Fv = np.ascontiguousarray(Q, np.float32), np.ascontiguousarray(F, np.float32)
        if Qv.ndim != 2 or Fv.ndim != 2 or Qv.shape[1] != Fv.shape[1]:
            raise ValueError("Q must be [N][K] and F [Kr][K]")
        N, Kr, K = self._admix_shape(Qv.shape[1])
        if Kr > 0 and (Qv.shape != (N, K) or Fv.shape != (Kr, K)):
            raise ValueError(f"Q must be [{N}][K] and F [{Kr}][K] (the samples and the kept rows of the handle)")
        mv = self._admix_mode(mode, N)
        Qn, Fn = np.zeros_like(Qv), np.zeros_like(Fv)
        ll, hl, nh, nhet = C.c_double(), C.c_double(), C.c_int64(), C.c_int64()
        self._chk(self._lib.gpca_admix_step_holdout(self._h, K, _vp(Qv), _vp(Fv), _vp(mv), int(folds), int(fold), int(cv_seed) & 0xffffffffffffffff,
                                                    _vp(Qn), _vp(Fn), C.byref(ll), C.byref(hl), C.byref(nh), C.byref(nhet)))
        return {"Q": Qn, "F": Fn, "loglik": ll.value, "held_loglik": hl.value, "n_held": int(nh.value), "n_het_held": int(nhet.value)}

    def admix_cv(self, K: int, folds: int = 5, cv_seed: int = 0, seed: int = 0, max_iter: int = 2000, tol: float = 1e-7, accel: bool = True,
                 mode=None, Q=None, F=None) -> dict:
        """The cross-validation error of the admixture fit with K ancestries (gpca_admix_cv; gpca.h section a22): per fold the fit of
        admix() with the fold's observed calls hidden in the step, then the hidden calls' binomial deviance at the fitted parameters.
        Starts every fold from admix_init(K, seed), or from Q and F when both are given.  Returns {"cv_error": the summed deviance over
        the summed n_held (NaN when nothing is held), "folds": one dict per fold of steps, cycles, converged, fallbacks, loglik (training),
        held_loglik, n_held, n_het_held, deviance}."""
        if (Q is None) != (F is None):
            raise ValueError("Q and F go together (both or neither)")
        N, Kr, K = self._admix_shape(K)
        Qv = Fv = None
        if Q is not None:
            Qv, Fv = np.ascontiguousarray(Q, np.float32), np.ascontiguousarray(F, np.float32)
            if Kr > 0 and (Qv.shape != (N, K) or Fv.shape != (Kr, K)):
                raise ValueError(f"Q must be [{N}][{K}] and F [{Kr}][{K}]")
        mv = self._admix_mode(mode, N)
        par = _lib.gpca_admix_params(K, int(max_iter), int(seed) & 0xffffffffffffffff, float(tol), 1 if accel else 0, 0 if Q is None else 1)
        out = (_lib.gpca_admix_cv_fold_info * max(min(int(folds), 64), 1))()
        cv = C.c_double()
        self._chk(self._lib.gpca_admix_cv(self._h, C.byref(par), _vp(mv), int(folds), int(cv_seed) & 0xffffffffffffffff, _vp(Qv), _vp(Fv), out,
                                          C.byref(cv)))
        rows = [{"steps": int(o.steps), "cycles": int(o.cycles), "converged": bool(o.converged), "fallbacks": int(o.fallbacks),
                 "loglik": o.loglik, "held_loglik": o.held_loglik, "n_held": int(o.n_held), "n_het_held": int(o.n_het_held),
                 "deviance": o.deviance} for o in out[:int(folds)]]
        return {"cv_error": cv.value, "folds": rows}

    @staticmethod
    def roh_threshold(x) -> Tuple[int, int]:
        """The window threshold as the ABI takes it: (num, den) = the exact fraction of x's decimal text (Fraction(str(x)): 0.05 is 1/20,
        not the binary double next to it).  x: a float, an int, a decimal or 'a/b' string, a Fraction, or a (num, den) pair, which is
        passed on as it is.  ValueError when the reduced denominator is above 2^20 or the value is not a finite number."""
        from fractions import Fraction
        if isinstance(x, tuple):
            if len(x) != 2:
                raise ValueError("window_threshold as a pair is (num, den)")
            return int(x[0]), int(x[1])
        try:
            fr = x if isinstance(x, Fraction) else Fraction(str(x))
        except (ValueError, ZeroDivisionError) as err:
            raise ValueError(f"window_threshold {x!r} is not a finite decimal number") from err
        if fr.denominator > _lib.ROH_DEN_MAX:
            raise ValueError(f"window_threshold {x!r} = {fr.numerator}/{fr.denominator}: the denominator is above 2^20")
        if abs(fr.numerator) >= 1 << 31:
            raise ValueError(f"window_threshold {x!r} is out of range")
        return fr.numerator, fr.denominator

    def roh(self, brk, window_snp: int = 50, window_het: int = 1, window_missing: int = 5, window_threshold=0.05, min_snp: int = 100,
            max_het: Optional[int] = None, rows: Optional[Tuple[int, int]] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Runs of homozygosity (gpca_roh; gpca.h section a20) over the kept rows [row0, row1) in PCA-SNP order (rows; default: all) and
        all samples.  brk: uint8, one per row of the band (io.roh_breaks): bit 0 = a window domain (chromosome) starts at the row,
        bit 1 = no run continues into the row.  A window of window_snp rows is a hit for a sample with at most window_het het and
        window_missing missing calls; a row is in a run iff the share of hits among the windows that cover it is at least
        window_threshold (roh_threshold); a run is reported with at least min_snp rows and at most max_het het calls (None: no limit).
        Returns (segs uint32 [n][5] = sample, first, last, n_het, n_missing in ascending (sample, first) order, first and last being
        kept-row indices of the handle; seg_count uint32 [N]).  Exact integers; a second call is made when the first buffer was short."""
        N = self.dims()[1]
        K = int(self._lib.gpca_num_pca_snps(self._h))
        r0, r1 = (0, K) if rows is None else (int(rows[0]), int(rows[1]))
        n = max(r1 - r0, 0)
        bv = np.asarray(brk)
        if bv.shape != (n,) or bv.dtype.kind not in "iub" or (bv.size and (int(bv.min()) < 0 or int(bv.max()) > 255)):
            raise ValueError("brk must be an unsigned byte array with one entry per row of the band")
        bb = np.zeros(max(n, 1), np.uint8)
        bb[:n] = bv
        num, den = self.roh_threshold(window_threshold)
        vals = (int(window_snp), int(window_het), int(window_missing), num, den, int(min_snp), -1 if max_het is None else int(max_het))
        if any(abs(v) >= 1 << 31 for v in vals):
            raise ValueError("a parameter of roh is outside 32 bits")
        if max_het is not None and int(max_het) < 0:
            raise ValueError("max_het must be None (no limit) or at least 0")
        par = _lib.gpca_roh_params(*vals)
        seg_count = np.zeros(max(N, 1), np.uint32)
        found = C.c_int64(0)
        cap = max(4 * N, 1024)
        while True:
            segs = np.zeros((cap, 5), np.uint32)
            self._chk(self._lib.gpca_roh(self._h, r0, r1, _vp(bb), C.byref(par), _vp(seg_count), _vp(segs), cap, C.byref(found)))
            if found.value <= cap:
                return segs[:found.value].copy(), seg_count[:N]
            cap = int(found.value)

    @staticmethod
    def roh_select(segs, positions, min_bp: int, max_bp_per_snp: int) -> np.ndarray:
        """The host rule on the records (gpca_roh_select; gpca.h section a20): segs [n][5] as roh gives them, positions [K] = the bp
        position of every kept row.  Returns uint8 [n]: 1 iff span = pos[last] - pos[first] >= min_bp and span <= max_bp_per_snp x
        (last - first + 1)."""
        sv = np.ascontiguousarray(segs, np.uint32)
        pv = np.ascontiguousarray(positions, np.int64)
        if sv.ndim != 2 or sv.shape[1] != 5 or pv.ndim != 1:
            raise ValueError("segs must be [n][5] as roh returns them and positions one entry per kept row")
        n = sv.shape[0]
        if n and int(sv[:, 1:3].max()) >= pv.shape[0]:
            raise ValueError("a record names a row beyond positions")
        keep = np.zeros(max(n, 1), np.uint8)
        lib = _lib.load()
        rc = lib.gpca_roh_select(_vp(sv if n else np.zeros((1, 5), np.uint32)), n, _vp(pv if pv.size else np.zeros(1, np.int64)),
                                 int(min_bp), int(max_bp_per_snp), _vp(keep))
        if rc != 0:
            raise GpcaError(rc, "gpca_roh_select: " + lib.gpca_status_string(rc).decode())
        return keep[:n]

    @staticmethod
    def het_weights(qc_counts) -> np.ndarray:
        """The rows' weights for the heterozygosity F (gpca_het_weights; host only; gpca.h section a18): qc_counts [rows][4] = n_valid,
        n_hom0, n_het, n_hom2 as snp_qc_detail gives them; returns uint32 [rows] = the unbiased expected heterozygosity of each row in
        units of 2^-30 (0 for a row without a call)."""
        cv = np.ascontiguousarray(qc_counts, np.uint32)
        if cv.ndim != 2 or cv.shape[1] != 4:
            raise ValueError("qc_counts must be [rows][4] as snp_qc_detail returns them")
        q = np.zeros(max(cv.shape[0], 1), np.uint32)
        lib = _lib.load()
        rc = lib.gpca_het_weights(_vp(cv if cv.shape[0] else np.zeros((1, 4), np.uint32)), cv.shape[0], _vp(q))
        if rc != 0:
            raise GpcaError(rc, "gpca_het_weights: " + lib.gpca_status_string(rc).decode())
        return q[:cv.shape[0]]

    @staticmethod
    def sample_het(counts, qsum) -> np.ndarray:
        """O_HOM, E_HOM and the inbreeding coefficient F of every sample (gpca_sample_het; host only; gpca.h section a18) from counts
        [N][3] and qsum [N] as sample_counts gives them with het_weights' weights, summed over the bands.  Returns float64 [N][3]; F is
        NaN for a sample without an observed call or without expected heterozygosity."""
        cv = np.ascontiguousarray(counts, np.uint32)
        qv = np.ascontiguousarray(qsum, np.uint64)
        if cv.ndim != 2 or cv.shape[1] != 3 or qv.shape != (cv.shape[0],):
            raise ValueError("counts must be [N][3] and qsum [N] as sample_counts returns them")
        N = cv.shape[0]
        out = np.zeros((max(N, 1), 3))
        lib = _lib.load()
        rc = lib.gpca_sample_het(_vp(cv if N else np.zeros((1, 3), np.uint32)), _vp(qv if N else np.zeros(1, np.uint64)), N, _vp(out))
        if rc != 0:
            raise GpcaError(rc, "gpca_sample_het: " + lib.gpca_status_string(rc).decode())
        return out[:N]

    @staticmethod
    def _fst_counts(counts):
        cv = np.ascontiguousarray(counts, np.uint32)
        if cv.ndim != 3 or cv.shape[2] != 3:
            raise ValueError("counts must be [rows][P][3] as group_counts returns them")
        return cv

    @staticmethod
    def fst_hudson(counts, sums=None, per_variant: bool = False):
        """Hudson's Fst of every pair of groups (gpca_fst_hudson; host only; gpca.h section a17) from counts [rows][P][3].  sums
        [P (P - 1) / 2][3] = the running sum of the numerators, of the denominators and the rows used per pair (j < i at
        i (i - 1) / 2 + j), ADDED TO in place when given (band after band), else started at zero.  Returns (fst [pairs] = sum num /
        sum den, NaN where that is 0 / 0, sums), and with per_variant=True also num, den [rows][pairs] (NaN where a group of the pair has
        no observed call)."""
        cv = GpcaEngine._fst_counts(counts)
        rows, P = cv.shape[0], cv.shape[1]
        pairs = P * (P - 1) // 2
        sv = np.zeros((max(pairs, 1), 3)) if sums is None else sums
        if sv.dtype != np.float64 or not sv.flags.c_contiguous or sv.shape != (max(pairs, 1), 3):
            raise ValueError("sums must be a C-contiguous float64 array [P (P - 1) / 2][3]")
        num = np.zeros((max(rows, 1), max(pairs, 1))) if per_variant else None
        den = np.zeros((max(rows, 1), max(pairs, 1))) if per_variant else None
        lib = _lib.load()
        rc = lib.gpca_fst_hudson(_vp(cv), rows, P, _vp(num), _vp(den), _vp(sv))
        if rc != 0:
            raise GpcaError(rc, "gpca_fst_hudson: " + lib.gpca_status_string(rc).decode())
        with np.errstate(invalid="ignore", divide="ignore"):
            fst = np.where(sv[:pairs, 1] != 0.0, sv[:pairs, 0] / sv[:pairs, 1], np.nan)
        return (fst, sv, num[:rows, :pairs], den[:rows, :pairs]) if per_variant else (fst, sv)

    @staticmethod
    def fst_wc(counts, use=None, sums=None, per_variant: bool = False):
        """Weir and Cockerham's Fst over the groups with use[p] != 0 (None: all; at least two) (gpca_fst_wc; host only; gpca.h section
        a17) from counts [rows][P][3].  sums [3] = the running sum of a, of a + b + c and the rows used, ADDED TO in place when given,
        else started at zero.  Returns (fst = sum a / sum (a + b + c), NaN for 0 / 0, sums), and with per_variant=True also abc
        [rows][3] (NaN where a used group has no observed call)."""
        cv = GpcaEngine._fst_counts(counts)
        rows, P = cv.shape[0], cv.shape[1]
        uv = None if use is None else np.ascontiguousarray(np.asarray(use) != 0, np.uint8)
        if uv is not None and uv.shape != (P,):
            raise ValueError("use must have one entry per group")
        sv = np.zeros(3) if sums is None else sums
        if sv.dtype != np.float64 or not sv.flags.c_contiguous or sv.shape != (3,):
            raise ValueError("sums must be a C-contiguous float64 array [3]")
        abc = np.zeros((max(rows, 1), 3)) if per_variant else None
        lib = _lib.load()
        rc = lib.gpca_fst_wc(_vp(cv), rows, P, _vp(uv), _vp(abc), _vp(sv))
        if rc != 0:
            raise GpcaError(rc, "gpca_fst_wc: " + lib.gpca_status_string(rc).decode())
        fst = float(sv[0] / sv[1]) if sv[1] != 0.0 else float("nan")
        return (fst, sv, abc[:rows]) if per_variant else (fst, sv)

    @staticmethod
    def logistic_null(y, covar=None, include=None):
        """The null logistic model of one case / control trait (gpca_logistic_null; host only): y [N] in {0, 1} on the included samples,
        covar [N][Pc] or None.  Returns (alpha [Pc + 1] in the coordinates of the standardised design, mu [N] with 0 outside the
        included samples, Newton steps); raises GpcaError (BAD_ARG: the inputs; NOT_CONVERGED: 25 steps or separation)."""
        yv = np.ascontiguousarray(y, np.float64).reshape(-1)
        N = yv.shape[0]
        Cv, inc = GpcaEngine._assoc_design(covar, include, N)
        Pc = Cv.shape[1]
        alpha, mu, it = np.zeros(Pc + 1), np.zeros(max(N, 1)), C.c_int32(0)
        lib = _lib.load()
        rc = lib.gpca_logistic_null(_vp(yv), _vp(Cv) if Pc else None, Pc, _vp(inc), N, _vp(alpha), _vp(mu), C.byref(it))
        if rc != 0:
            raise GpcaError(rc, "gpca_logistic_null: " + lib.gpca_status_string(rc).decode())
        return alpha, mu[:N], int(it.value)

    @staticmethod
    def spa_log10p(gt, mu, u: float):
        """The saddle-point correction for one given vector (gpca_spa_log10p; host only): gt [n] = the genotype with the covariates
        taken out, mu [n] = the null model's probabilities, u = the score sum gt (y - mu).  Returns (-log10 of the two-sided p,
        status, (zeta+, zeta-)): status 0 for u = 0 (p = 1), 1 for the correction, 2 where a tail did not converge or failed (the
        normal value of u / sqrt(sum mu (1 - mu) gt^2))."""
        gv, mv = np.ascontiguousarray(gt, np.float64).reshape(-1), np.ascontiguousarray(mu, np.float64).reshape(-1)
        if gv.shape != mv.shape:
            raise ValueError("gt and mu must have one entry per sample each")
        lp, zeta, st = C.c_double(0.0), np.zeros(2), C.c_int32(0)
        lib = _lib.load()
        rc = lib.gpca_spa_log10p(_vp(gv), _vp(mv), gv.shape[0], float(u), C.byref(lp), _vp(zeta), C.byref(st))
        if rc != 0:
            raise GpcaError(rc, "gpca_spa_log10p: " + lib.gpca_status_string(rc).decode())
        return float(lp.value), int(st.value), (float(zeta[0]), float(zeta[1]))

    @staticmethod
    def firth_log10p(gt, mu, u: float):
        """The approximate Firth correction for one given vector (gpca_firth_log10p; host only): gt, mu and u as for spa_log10p.
        Returns (-log10 p, status, beta, se, lrt): status 1 for the correction, 2 where the root rule failed (the normal value of
        u / sqrt(sum mu (1 - mu) gt^2); beta, se and lrt what was reached).  There is no cutoff."""
        gv, mv = np.ascontiguousarray(gt, np.float64).reshape(-1), np.ascontiguousarray(mu, np.float64).reshape(-1)
        if gv.shape != mv.shape:
            raise ValueError("gt and mu must have one entry per sample each")
        out = np.zeros(5)
        lib = _lib.load()
        rc = lib.gpca_firth_log10p(_vp(gv), _vp(mv), gv.shape[0], float(u), _vp(out))
        if rc != 0:
            raise GpcaError(rc, "gpca_firth_log10p: " + lib.gpca_status_string(rc).decode())
        return float(out[0]), int(out[1]), float(out[2]), float(out[3]), float(out[4])

    @staticmethod
    def normal_log10p(z: float) -> float:
        """-log10 of the two-sided p-value of a standard normal statistic (gpca_normal_log10p; host only, no underflow)."""
        return float(_lib.load().gpca_normal_log10p(float(z)))

    # -- f3: the stages of EigenSNPCoreAlgorithm (gpca.h)
    def copy_rows_from(self, src: "GpcaEngine", row0: int, rows: int):
        """This engine receives rows [row0, row0 + rows) of src's resident matrix (device to device)."""
        self._chk(self._lib.gpca_copy_rows(self._h, src._h, row0, rows))

    def set_sample_mask(self, mask: Optional[np.ndarray]):
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        if m is not None and m.shape != (self.dims()[1],):
            raise ValueError("mask must have one entry per sample")
        self._chk(self._lib.gpca_set_sample_mask(self._h, _vp(m)))

    def set_condensed_basis(self, W: np.ndarray, feat0: np.ndarray, R: int):
        W = np.ascontiguousarray(W, np.float32); feat0 = np.ascontiguousarray(feat0, np.int32)
        M, _ = self.dims()
        if W.ndim != 2 or W.shape[0] != M or feat0.shape != (M,):
            raise ValueError("W must be [SNPs, cmax] and feat0 [SNPs]")
        self._chk(self._lib.gpca_set_condensed_basis(self._h, _vp(W), _vp(feat0), W.shape[1], R))

    def rsvd_condensed(self, k: int, oversample: int = 10, power_iters: int = 2, seed: int = 1):
        self._chk(self._lib.gpca_rsvd_condensed(self._h, k, oversample, power_iters, seed))
        self._k, self._l = k, k + oversample

    def refine(self, scores: np.ndarray):
        s = np.ascontiguousarray(scores, np.float64)
        if s.ndim != 2 or s.shape[0] != self.dims()[1]:
            raise ValueError("scores must be [samples, k]")
        self._chk(self._lib.gpca_refine(self._h, _vp(s), s.shape[1]))
        self._k = self._l = s.shape[1]

    # -- e
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(_lib.GPCA_UNIQUE_ID_BYTES)
        rc = _lib.load().gpca_comm_get_unique_id(buf)
        if rc != _lib.GPCA_OK:
            raise GpcaError(rc, _lib.load().gpca_last_error(None).decode())
        return buf.raw

    def comm_init(self, world: int, rank: int, unique_id: bytes, snp_offset: int):
        self._chk(self._lib.gpca_comm_init(self._h, world, rank, C.c_char_p(unique_id), snp_offset))

    def comm_count_ranks(self) -> int:
        """Ranks the exchange actually reaches (collective: a 1.0 per rank summed through RCCL or the hook)."""
        n = C.c_int32()
        self._chk(self._lib.gpca_comm_count_ranks(self._h, C.byref(n)))
        return n.value

    def set_allreduce_hook(self, fn, world: int, rank: int, snp_offset: int):
        """fn(np.ndarray f64 view) sums the buffer in place across ranks (any transport)."""
        def _tramp(_user, ptr, count):
            try:
                fn(np.ctypeslib.as_array(ptr, shape=(count,)))
                return 0
            except Exception:  # pragma: no cover
                return 1
        self._hook_ref = _lib.ALLREDUCE_FN(_tramp)
        self._chk(self._lib.gpca_set_allreduce_hook(self._h, self._hook_ref, None, world, rank, snp_offset))

    # -- d
    def reset_timings(self):
        self._chk(self._lib.gpca_reset_timings(self._h))

    def enable_timings(self, on):
        """True / 1: HIP events around every timed kernel; n > 1: only every n-th rsvd call records them (the others run without the
        ~5 us of idle stream an event pair costs); False / 0: off."""
        self._chk(self._lib.gpca_enable_timings(self._h, int(on)))

    def timings(self) -> dict:
        n = C.c_int32()
        arr = (_lib.gpca_kernel_timing * 32)()
        self._chk(self._lib.gpca_get_timings(self._h, arr, 32, C.byref(n)))   # (timings are off until enable_timings(True))
        return {arr[i].name.decode(): dict(launches=arr[i].launches, total_ms=arr[i].total_ms, flops=arr[i].flops,
                                           bytes=arr[i].bytes) for i in range(min(n.value, 32))}

    def synchronize(self):
        self._chk(self._lib.gpca_synchronize(self._h))


def _digest_i8(g: np.ndarray) -> bytes:
    """Identity of an int8 genotype matrix (PCA.transform(x) recognises the fitted matrix by it)."""
    import hashlib
    h = hashlib.blake2b(digest_size=32)
    h.update(np.asarray(g.shape, np.int64).tobytes())
    h.update(np.ascontiguousarray(g).data)
    return h.digest()


def _dosages_snp_major(x: np.ndarray, where: str) -> np.ndarray:
    """samples x variants dosages (0/1/2; NaN = missing) -> int8 SNP-major rows with -127 for a missing call."""
    n_samples, n_features = x.shape
    if x.dtype == np.int8:
        return np.ascontiguousarray(x.T)
    g = np.empty((n_features, n_samples), np.int8)
    step = max(1, (1 << 24) // max(n_features, 1))
    for s0 in range(0, n_samples, step):
        blk = np.asarray(x[s0:s0 + step], np.float64)
        miss = np.isnan(blk)
        r = np.rint(np.where(miss, 0.0, blk))
        if not (np.all(np.abs(r) <= 127) and np.array_equal(r[~miss], blk[~miss])):
            raise ValueError(f"{where}: x must hold genotype dosages 0/1/2 or NaN (found a value that is not a whole number)")
        r[miss] = -127
        g[:, s0:s0 + step] = r.T.astype(np.int8)
    return g


# ------------------------------------------------------------------------------------------------
# efficient_pca::PCA as called at main.rs:602, 648-660
# ------------------------------------------------------------------------------------------------
class PCA:
    """``PCA::new()``, ``.rfit(x, k, n_oversamples, seed, tol)``, ``.transform(x)``.

    ``x`` is samples x variants (vcf.rs:329-342 orientation) with dosages 0/1/2.  The device keeps
    it as int8 SNP-major (1 B/genotype instead of build_matrix's 8 B + clone, main.rs:640).
    Standardisation: column mean and sample (n-1) standard deviation (UNVERIFIED for the
    un-vendored crate; matches the in-tree BED path prepare.rs:1294,1357-1364).  ``tol`` is
    accepted for signature parity and ignored (main.rs:638 always passes None).
    """

    def __init__(self, device: int = -1, precision: int = _lib.PREC_I8_EXACT, storage: int = _lib.STORE_INT8):
        self._eng = GpcaEngine(device=device, precision=precision, storage=storage)
        self._fitted = False

    def rfit(self, x: np.ndarray, k: int, n_oversamples: int = 10, seed: Optional[int] = None, tol=None,
             power_iters: int = 2):
        x = np.asarray(x)
        if x.ndim != 2:
            raise ValueError("x must be samples x variants")
        n_samples, n_features = x.shape
        if k == 0:
            raise ValueError("Number of components (-k) must be > 0.")          # main.rs:607-609
        if n_samples < 2:
            raise ValueError(f"PCA requires at least 2 samples, found {n_samples}.")  # main.rs:614-616
        if n_features == 0:
            raise ValueError("PCA requires at least 1 variant (feature), found 0.")   # main.rs:617-619
        k = min(k, n_samples, n_features)                                              # main.rs:621-628
        if x.dtype == np.int8:
            g = np.ascontiguousarray(x.T)
        else:
            # build_matrix (vcf.rs:317-345) fills x with u8 dosages; this engine keeps them as codes, so anything that is not
            # a whole number in the int8 range is refused here (values other than 0/1/2 are refused by the device, status -9)
            g = np.empty((n_features, n_samples), np.int8)
            step = max(1, (1 << 24) // max(n_features, 1))
            for s0 in range(0, n_samples, step):
                blk = np.asarray(x[s0:s0 + step])
                r = np.rint(blk)
                if not (np.all(np.abs(r) <= 127) and np.array_equal(r, blk)):
                    raise ValueError("PCA.rfit: x must hold genotype dosages 0/1/2 (found a value that is not a whole number)")
                g[:, s0:s0 + step] = r.T.astype(np.int8)
        self._eng.upload_genotypes_i8(g)
        self._fit_digest = _digest_i8(g)
        self._n_features = n_features
        self._eng.snp_stats(QcConfig.none(), fetch=False)
        # zero-variance rows leave the PCA even without QC thresholds: the reference's clamp (main.rs:621-628), applied to what is left
        if self._eng.num_pca_snps() == 0:
            raise ValueError("PCA requires at least 1 variant (feature), found 0.")
        k = min(k, self._eng.num_pca_snps())
        l = min(k + n_oversamples, n_samples, self._eng.num_pca_snps())
        self._eng.rsvd(k, l - k, power_iters, 0 if seed is None else int(seed))
        self._fitted = True
        self.k = k
        return self

    def transform(self, x: Optional[np.ndarray] = None) -> np.ndarray:
        """Scores of samples x variants ``x`` on the fitted axes.  No ``x``, or the fitted matrix itself: the fitted matrix's scores (the
        reference passes the clone of the same x, main.rs:640,659).  Any other ``x`` with the fitted variant count (NaN = missing call)
        is projected with the fitted mean, s.d. and loadings through a second engine (gpca_project; missing calls mean-imputed)."""
        if not self._fitted:
            raise RuntimeError("PCA.transform before rfit")
        if x is None:
            return self._eng.transform()
        x = np.asarray(x)
        if x.ndim != 2 or x.shape[1] != self._n_features:
            raise ValueError(f"PCA.transform: x must be samples x {self._n_features} variants, got shape {x.shape}")
        g = _dosages_snp_major(x, "PCA.transform")
        if _digest_i8(g) == self._fit_digest:
            return self._eng.transform()
        st = self._eng.get_standardization()
        W = np.zeros((self._n_features, self.k), np.float32)
        W[self._eng.pca_snp_rows()] = self._eng.loadings()
        with GpcaEngine(device=self._eng._device, precision=_lib.PREC_I8_EXACT, storage=self._eng.storage) as e:
            e.upload_genotypes_i8(g)
            return e.project(st["mu"], st["sigma"], W)[0]

    def explained_variance(self) -> np.ndarray:
        return self._eng.eigenvalues()

    def rotation(self) -> np.ndarray:
        return self._eng.loadings()


# ------------------------------------------------------------------------------------------------
# The L2 boundary types, prepare.rs:1771-2030
# ------------------------------------------------------------------------------------------------
@dataclass
class LdBlockSpecification:
    user_defined_block_tag: str
    pca_snp_ids_in_block: list


class MicroarrayGenotypeAccessor:
    """``impl PcaReadyGenotypeAccessor for MicroarrayGenotypeAccessor`` (prepare.rs:1838-2030),
    backed by genotypes resident in HBM instead of the IoService actor pool."""

    def __init__(self, engine: GpcaEngine):
        self.engine = engine

    def get_standardized_snp_sample_block(self, pca_snp_ids_to_fetch, qc_sample_ids_to_fetch) -> np.ndarray:
        return self.engine.standardize_block(pca_snp_ids_to_fetch, qc_sample_ids_to_fetch)

    def num_pca_snps(self) -> int:
        return self.engine.num_pca_snps()

    def num_qc_samples(self) -> int:
        return self.engine.num_qc_samples()

    def original_indices_of_pca_snps(self) -> np.ndarray:
        return self.engine.pca_snp_rows()


@dataclass
class EigenSNPCoreAlgorithmConfig:
    """The 14 fields of main.rs:311-327 with clap's effective defaults (main.rs:561-588)."""
    target_num_global_pcs: int = 10
    components_per_ld_block: int = 7
    subset_factor_for_local_basis_learning: float = 0.075
    min_subset_size_for_local_basis_learning: int = 10_000
    max_subset_size_for_local_basis_learning: int = 40_000
    global_pca_sketch_oversampling: int = 10
    global_pca_num_power_iterations: int = 2
    local_rsvd_sketch_oversampling: int = 10
    local_rsvd_num_power_iterations: int = 2
    random_seed: int = 2025
    snp_processing_strip_size: int = 2000
    refine_pass_count: int = 1
    collect_diagnostics: bool = False
    diagnostic_block_list_id_to_trace: Optional[int] = None


@dataclass
class EigenSNPCoreOutput:
    final_sample_principal_component_scores: np.ndarray   # [N, K] f32   main.rs:389
    final_principal_component_eigenvalues: np.ndarray     # [K] f64      main.rs:394
    final_snp_principal_component_loadings: np.ndarray    # [D, K] f32   main.rs:407
    num_qc_samples_used: int = 0
    num_pca_snps_used: int = 0
    num_principal_components_computed: int = 0
    # compute_pca(..., project_all=True): every sample projected onto the fit (gpca_transform, [N, K] f64), taken while the fit is
    # valid -- before the keep mask of the blocks' union is restored (which drops the fit)
    projected_sample_scores: Optional[np.ndarray] = None


class EigenSNPCoreAlgorithm:
    """``EigenSNPCoreAlgorithm::new(cfg).compute_pca(&accessor, &blocks)`` (main.rs:359-365).

    Two ways to the same quantity (top-K PCA of the standardised matrix restricted to the SNPs the caller's ``ld_blocks`` name --
    a PCA SNP in no block does not enter, prepare.rs:1465-1469):

    * ``local_stage=False`` (default): ONE global randomized PCA over the union of the blocks -- what the GPU does best (6 passes
      over the genotypes, every power iteration on the full matrix) and the more accurate of the two.  Acting config fields:
      ``target_num_global_pcs``, ``global_pca_sketch_oversampling``, ``global_pca_num_power_iterations``, ``random_seed``.
    * ``local_stage=True``: the multi-stage algorithm the 14 config fields (main.rs:311-327) parameterise, as published for the
      un-vendored ``efficient_pca`` crate (Cargo.toml:30, no pinned revision -- parity UNPINNED):
        1. a sample subset of ``clamp(subset_factor * N, min_subset, max_subset)`` samples (seeded);
        2. per LD block, a local randomized PCA on the subset's columns -> ``components_per_ld_block`` local eigenSNP loadings
           (``local_rsvd_sketch_oversampling`` / ``local_rsvd_num_power_iterations``);
        3. every sample projected on the local bases -> condensed features, row-standardised;
        4. an initial global randomized PCA of the condensed features (``global_pca_*``) -> sample scores;
        5. ``refine_pass_count`` refinement passes on the full matrix: loadings = orth(X scores), scores = X^T loadings, small SVD.
      Every pass over genotypes runs on the device (gpca.h section f3); the host only assembles the block-diagonal basis.
      ``snp_processing_strip_size`` stays a no-op (HBM-resident rows); ``collect_diagnostics`` returns a small dict of what ran.
    """

    def __init__(self, config: EigenSNPCoreAlgorithmConfig):
        self.config = config

    @staticmethod
    def _union_of_blocks(ld_blocks: Sequence[LdBlockSpecification], n_pca: int) -> np.ndarray:
        if len(ld_blocks) == 0:
            raise ValueError("compute_pca: ld_block_specifications is empty")
        ids = np.unique(np.concatenate([np.asarray(b.pca_snp_ids_in_block, np.int64).reshape(-1) for b in ld_blocks]))
        if ids.size == 0:
            raise ValueError("compute_pca: the LD blocks hold no PCA SNP")
        if ids[0] < 0 or ids[-1] >= n_pca:
            raise ValueError(f"compute_pca: PcaSnpId {int(ids[0] if ids[0] < 0 else ids[-1])} out of range [0, {n_pca})")
        return ids

    def compute_pca(self, accessor: MicroarrayGenotypeAccessor, ld_blocks: Sequence[LdBlockSpecification], local_stage: bool = False,
                    project_all: bool = False):
        eng = accessor.engine
        cfg = self.config
        n_pca = accessor.num_pca_snps()
        ids = self._union_of_blocks(ld_blocks, n_pca)
        restore = None
        if ids.size < n_pca or local_stage:
            # SNPs outside every block leave the PCA: keep mask = union of the blocks (same mu/sigma); the accessor's
            # own PCA-SNP numbering is restored afterwards, as the reference never mutates its accessor
            st = eng.get_standardization()
            rows = eng.pca_snp_rows()
            keep2 = np.zeros_like(st["keep"])
            keep2[rows[ids]] = 1
            if ids.size < n_pca:
                eng.set_standardization(st["mu"], st["sigma"], keep2)
                restore = st
        diag = None
        try:
            if local_stage:
                diag = self._multi_stage(eng, ld_blocks, st, rows)
            else:
                eng.rsvd(cfg.target_num_global_pcs, cfg.global_pca_sketch_oversampling, cfg.global_pca_num_power_iterations,
                         cfg.random_seed)
            sc = eng.scores()     # (the local stage may leave fewer components than target_num_global_pcs: min(K, condensed features))
            out = EigenSNPCoreOutput(sc, eng.eigenvalues(), eng.loadings(), accessor.num_qc_samples(),
                                     int(ids.size), int(sc.shape[1]), eng.transform() if project_all else None)
        finally:
            if restore is not None:
                eng.set_standardization(restore["mu"], restore["sigma"], restore["keep"])
        if cfg.collect_diagnostics:
            diag = dict(diag or {}, stage="multi-stage" if local_stage else "global", num_ld_blocks=len(ld_blocks),
                        num_pca_snps_in_blocks=int(ids.size), pca_snp_ids_used=ids)
        else:
            diag = None
        return out, diag

    # ---- the multi-stage algorithm ---------------------------------------------------------------------------------
    @staticmethod
    def subset_size(cfg: EigenSNPCoreAlgorithmConfig, n_samples: int) -> int:
        want = int(round(cfg.subset_factor_for_local_basis_learning * n_samples))
        want = max(cfg.min_subset_size_for_local_basis_learning, min(cfg.max_subset_size_for_local_basis_learning, want))
        return max(2, min(n_samples, want))

    @staticmethod
    def subset_mask(cfg: EigenSNPCoreAlgorithmConfig, n_samples: int) -> Optional[np.ndarray]:
        """Seeded sample subset for the local bases (None = every sample): the first ns entries of a Fisher-Yates shuffle driven
        by SplitMix64(seed) -- defined here rather than taken from a library generator so that the C++ host (gpca.hpp) draws the
        same samples.  The crate uses ChaCha: WHICH samples are drawn cannot match the reference, only how many."""
        ns = EigenSNPCoreAlgorithm.subset_size(cfg, n_samples)
        if ns >= n_samples:
            return None
        m64 = (1 << 64) - 1
        state = cfg.random_seed & m64
        idx = list(range(n_samples))
        for i in range(ns):
            state = (state + 0x9E3779B97F4A7C15) & m64
            z = state
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m64
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m64
            z ^= z >> 31
            j = i + z % (n_samples - i)
            idx[i], idx[j] = idx[j], idx[i]
        mask = np.zeros(n_samples, np.uint8); mask[idx[:ns]] = 1
        return mask

    def _multi_stage(self, eng: "GpcaEngine", ld_blocks, st, pca_rows):
        cfg = self.config
        M, N = eng.dims()
        K = cfg.target_num_global_pcs
        mask = self.subset_mask(cfg, N)
        n_sub = N if mask is None else int(mask.sum())
        blocks = [(b.user_defined_block_tag, np.sort(pca_rows[np.asarray(b.pca_snp_ids_in_block, np.int64)])) for b in ld_blocks
                  if len(b.pca_snp_ids_in_block)]
        cp = max(1, cfg.components_per_ld_block)
        # stages 1-3: local bases on the subset, all samples projected, feature standard deviations
        cmax = min(cp, max(len(r) for _, r in blocks), n_sub)
        W = np.zeros((M, cmax), np.float32)
        feat0 = np.full(M, -1, np.int32)
        R = 0
        kw = dict(device=eng._device, precision=eng.precision, storage=eng.storage, digit_planes=eng.digit_planes)
        with GpcaEngine(**kw) as sub:
            big = max(blocks, key=lambda b: int(b[1][-1]) - int(b[1][0]))[1]
            sub.copy_rows_from(eng, int(big[0]), int(big[-1]) + 1 - int(big[0]))     # sized once for the widest block: every block reuses its buffers
            for bi, (_, rows) in enumerate(blocks):
                r0, r1 = int(rows[0]), int(rows[-1]) + 1
                sub.copy_rows_from(eng, r0, r1 - r0)
                keep = np.zeros(r1 - r0, np.uint8); keep[rows - r0] = 1
                sub.set_standardization(st["mu"][r0:r1], st["sigma"][r0:r1], keep)
                sub.set_sample_mask(mask)
                c = min(cp, len(rows), n_sub)
                lo = max(0, min(cfg.local_rsvd_sketch_oversampling, min(len(rows), n_sub) - c))
                sub.rsvd(c, lo, cfg.local_rsvd_num_power_iterations, cfg.random_seed + 1 + bi)
                U = sub.loadings()                                   # [block SNPs, c], orthonormal columns
                feats = sub.transform()                              # [N, c]: every sample on the local basis
                sd = feats.std(axis=0, ddof=1)
                ok = sd > 1e-12
                U = U[:, ok] / sd[ok].astype(np.float32)
                c = U.shape[1]
                if c == 0:
                    continue
                W[rows, :c] = U
                feat0[rows] = R
                R += c
        if R < 1:
            raise ValueError("compute_pca: no condensed features (every local component is constant)")
        # stage 4: initial global PCs from the condensed features (never formed on the host)
        eng.set_sample_mask(None)
        eng.set_condensed_basis(W, feat0, R)
        k0 = min(K, R)
        go = max(0, min(cfg.global_pca_sketch_oversampling, min(R, N) - k0))
        eng.rsvd_condensed(k0, go, cfg.global_pca_num_power_iterations, cfg.random_seed)
        scores = eng.scores(f64=True)
        # stage 5: refinement on the full matrix
        for _ in range(max(1, cfg.refine_pass_count)):
            eng.refine(scores)
            scores = eng.scores(f64=True)
        return dict(num_condensed_features=R, subset_size=n_sub, refine_passes=max(1, cfg.refine_pass_count))


