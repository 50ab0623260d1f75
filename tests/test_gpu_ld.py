"""gpca_ld_window: windowed pairwise r^2 of the kept rows (ld.hip, gpca_ld.cpp), through the C ABI.

The semantics every layer implements, restated in numpy (``ref_ld``) from the genotypes.  For a pair i < j of kept rows and sample n,
with o = [call observed] and g' = g on an observed call, 0 on a missing one:
    n = sum o_i o_j,  sx = sum g'_i o_j,  sy = sum o_i g'_j,  sxx = sum g'_i^2 o_j,  syy = sum o_i g'_j^2,  sxy = sum g'_i g'_j
    cov = n sxy - sx sy,  vx = n sxx - sx sx,  vy = n syy - sy sy,  r2 = (cov cov) / (vx vy)   (NaN when vx <= 0 or vy <= 0)
Every intermediate but the two products and the division is an exact integer in f64, so the device gives the same bits: every
comparison below is exact."""
import os
import threading

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from genomic_pca_amd import io as gio
from genomic_pca_amd._lib import GpcaError
from _edges import EDGE_N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORES = {"int8": _lib.STORE_INT8, "2bit": _lib.STORE_2BIT}
WMAX = [1, 31, 32, 33, 50, 64, 200, 1000]


def genotypes(M, N, seed, miss=0.0, special=True):
    """LD by construction: each row copies the row before it on most samples.  special: a constant row, an all-missing row and two
    neighbouring rows never observed together (each forces NaN in its pairs)."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.5, size=(M, 1))
    G = (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)
    for i in range(1, M):
        if i % 7:
            cp = rng.random(N) < 0.7
            G[i, cp] = G[i - 1, cp]
    if miss > 0:
        G[rng.random((M, N)) < miss] = -127
    if special and M >= 40:
        G[M // 3] = 1
        G[M // 2] = -127
        a = 2 * M // 3
        G[a, N // 2:] = -127
        G[a + 1, :N // 2] = -127
    return G


def ref_ld(G, keep, win_end, wmax, row0=0, row1=None):
    """(r2 [rows][wmax] f64, counts [rows][wmax][6] int32) of kept rows [row0, row1): the restatement of the module docstring.  The six
    sums come from f32 matrix products of small integers (every partial sum is an integer below 2^24: exact)."""
    X = G[np.asarray(keep).astype(bool)]
    K, N = X.shape
    row1 = K if row1 is None else row1
    rows = row1 - row0
    assert 4 * N < 2 ** 24
    o = (X != -127)
    g = np.where(o, X, 0).astype(np.float32)
    q = g * g
    o = o.astype(np.float32)
    pad = np.zeros((wmax + 1, N), np.float32)
    g, q, o = (np.concatenate([a, pad]) for a in (g, q, o))
    cnt = np.zeros((rows, wmax, 6), np.int32)
    B = 256
    d = np.arange(wmax)
    for b0 in range(row0, row1, B):
        b1 = min(b0 + B, row1)
        t = np.arange(b1 - b0)
        col = t[:, None] + d[None, :]
        A, C = slice(b0, b1), slice(b0 + 1, b1 + wmax)
        prods = (o[A] @ o[C].T, g[A] @ o[C].T, o[A] @ g[C].T, q[A] @ o[C].T, o[A] @ q[C].T, g[A] @ g[C].T)
        for s, P in enumerate(prods):
            cnt[b0 - row0:b1 - row0, :, s] = P[t[:, None], col].astype(np.int32)
    inwin = (np.arange(row0, row1)[:, None] + 1 + d[None, :]) < np.asarray(win_end, np.int64)[:, None]
    cnt[~inwin] = 0
    c = cnt.astype(np.float64)
    n, sx, sy, sxx, syy, sxy = (c[..., s] for s in range(6))
    cov, vx, vy = n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy
    with np.errstate(divide="ignore", invalid="ignore"):
        r2 = (cov * cov) / (vx * vy)
    r2[(vx <= 0) | (vy <= 0)] = np.nan
    r2[~inwin] = 0.0
    return r2, cnt


def count_windows(K, w, row0=0, row1=None):
    row1 = K if row1 is None else row1
    return np.minimum(np.arange(row0, row1, dtype=np.int64) + 1 + w, K)


def unpack(above, wmax):
    return np.unpackbits(np.ascontiguousarray(above).view(np.uint8), axis=1, bitorder="little")[:, :wmax].astype(bool)


def load(e, G, keep=None):
    M = G.shape[0]
    e.upload_genotypes_i8(G)
    e.snp_stats(gpca.QcConfig.none())
    keep = np.ones(M, np.uint8) if keep is None else keep
    e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), keep)
    return keep


def check(e, G, keep, win_end, wmax, thr=0.2, ref=None):
    out = e.ld_window(win_end, wmax=wmax, threshold=thr, counts=True)
    r2, cnt = ref if ref is not None else ref_ld(G, keep, win_end, wmax)
    assert out["counts"].shape == cnt.shape and out["r2"].shape == r2.shape
    assert np.array_equal(out["counts"], cnt)
    assert np.array_equal(out["r2"], r2, equal_nan=True)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(unpack(out["above"], wmax), r2 > thr)
    return out


# 1. parity with numpy: counts exact, r2 bit for bit, every wmax; rows that force NaN are kept through set_standardization
@pytest.mark.parametrize("store", ["int8", "2bit"])
@pytest.mark.parametrize("miss", [0.0, 0.02])
@pytest.mark.parametrize("N", EDGE_N + [200, 1500, 2085])
def test_matches_numpy(store, N, miss):
    M = 3000
    G = genotypes(M, N, seed=N + int(miss * 100), miss=miss)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        keep = load(e, G)
        full = ref_ld(G, keep, count_windows(M, max(WMAX)), max(WMAX))
        nan_rows = 0
        for w in WMAX:
            we = count_windows(M, w)
            inwin = (np.arange(M)[:, None] + 1 + np.arange(w)[None, :]) < we[:, None]
            ref = (np.where(inwin, full[0][:, :w], 0.0), np.where(inwin[..., None], full[1][:, :w], 0))
            out = check(e, G, keep, we, w, ref=ref)
            nan_rows = int(np.isnan(out["r2"][[M // 3, M // 2]]).all(axis=1).sum())
            assert np.isnan(out["r2"][2 * M // 3, 0]) and out["counts"][2 * M // 3, 0, 0] == 0      # never observed together: n = 0
        assert nan_rows == 2                                         # the constant and the all-missing row: NaN across the window


# 2. a scattered keep mask: windows are counted in kept rows
@pytest.mark.parametrize("store", ["int8", "2bit"])
@pytest.mark.parametrize("frac", [0.9, 0.05])
def test_scattered_keep(store, frac):
    M, N = 6000, 700
    G = genotypes(M, N, seed=5, miss=0.02)
    keep = (np.random.default_rng(6).random(M) < frac).astype(np.uint8)
    K = int(keep.sum())
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        load(e, G, keep)
        assert np.array_equal(e.pca_snp_rows(), np.flatnonzero(keep))
        for w in (50, 333):
            check(e, G, keep, count_windows(K, w), w)


# 3. row bands (a one-row band and the last row included) concatenate to the full call bit for bit
@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_bands_bit_identical(store):
    M, N, w = 2500, 900, 100
    G = genotypes(M, N, seed=7, miss=0.02)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        load(e, G)
        we = count_windows(M, w)
        full = e.ld_window(we, wmax=w, threshold=0.3, counts=True)
        cuts = [0, 1, 2, 63, 64, 65, 700, 701, 1999, M - 1, M]
        parts = [e.ld_window(we[a:b], wmax=w, rows=(a, b), threshold=0.3, counts=True) for a, b in zip(cuts[:-1], cuts[1:])]
        assert parts[0]["r2"].shape == (1, w) and parts[-1]["r2"].shape == (1, w) and not parts[-1]["counts"].any()
        for key in ("r2", "counts", "above"):
            assert np.array_equal(np.concatenate([p[key] for p in parts]), full[key], equal_nan=key == "r2"), key
        empty = e.ld_window(we[:0], wmax=w, rows=(5, 5))
        assert empty["r2"].shape == (0, w)


# 4. ragged windows: two chromosome boundaries and kb-style variable widths; slots outside a row's window are 0 everywhere
@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_ragged_windows(store):
    M, N = 3000, 500
    G = genotypes(M, N, seed=9, miss=0.02)
    rng = np.random.default_rng(10)
    chrom = np.repeat(["1", "2", "3"], [900, 1300, 800])
    pos = np.concatenate([np.sort(rng.integers(1, 3_000_000, n)) for n in (900, 1300, 800)])
    we = gio.ld_windows(chrom, pos, "150kb")
    wmax = int(np.max(we - np.arange(M) - 1))
    assert we[899] == 900 and we[2199] == 2200 and we[-1] == M and wmax > 64
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        keep = load(e, G)
        out = check(e, G, keep, we, wmax + 3)
        outside = (np.arange(M)[:, None] + 1 + np.arange(wmax + 3)[None, :]) >= we[:, None]
        assert not out["r2"][outside].any() and not out["counts"][outside].any() and not unpack(out["above"], wmax + 3)[outside].any()
        check(e, G, keep, gio.ld_windows(chrom, pos, "50"), 49)


# 5. above = (r2 > threshold) packed, NaN slots and padding bits 0, with r2 NULL as well
@pytest.mark.parametrize("store", ["int8", "2bit"])
@pytest.mark.parametrize("w", [50, 64, 130])
def test_above_bits(store, w):
    M, N = 2000, 300
    G = genotypes(M, N, seed=11, miss=0.02)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        keep = load(e, G)
        we = count_windows(M, w)
        r2, _ = ref_ld(G, keep, we, w)
        inwin = (np.arange(M)[:, None] + 1 + np.arange(w)[None, :]) < we[:, None]
        for thr in (0.0, 0.2, 0.5, 1.0, -1.0):
            both = e.ld_window(we, wmax=w, threshold=thr)
            only = e.ld_window(we, wmax=w, threshold=thr, r2=False)
            assert set(only) == {"above"} and np.array_equal(only["above"], both["above"])
            bits = np.unpackbits(only["above"].view(np.uint8), axis=1, bitorder="little").astype(bool)
            with np.errstate(invalid="ignore"):
                assert np.array_equal(bits[:, :w], (r2 > thr) & inwin)     # (a slot outside the window is 0 even below a negative threshold)
            assert not bits[:, w:].any()                           # padding bits
            assert not bits[:, :w][np.isnan(r2)].any()             # NaN is not above
        assert np.isnan(r2).any()


# 6. int8 == 2-bit; the other precision of the handle gives the same bits; few rows x many samples (the sample-axis split)
def test_storage_precision_and_sample_split():
    M, N, w = 1500, 1100, 70
    G = genotypes(M, N, seed=13, miss=0.02)
    we = count_windows(M, w)
    outs = []
    for prec in (_lib.PREC_I8_EXACT, _lib.PREC_F32_MFMA):
        for store in ("int8", "2bit"):
            with gpca.GpcaEngine(precision=prec, storage=STORES[store]) as e:
                load(e, G)
                outs.append(e.ld_window(we, wmax=w, threshold=0.2, counts=True))
    for o in outs[1:]:
        for key in ("r2", "counts", "above"):
            assert np.array_equal(o[key], outs[0][key], equal_nan=key == "r2"), key
    M, N, w = 96, 40000, 40
    G = genotypes(M, N, seed=14, miss=0.01)
    we = count_windows(M, w)
    for store in ("int8", "2bit"):
        with gpca.GpcaEngine(storage=STORES[store]) as e:
            keep = load(e, G)
            check(e, G, keep, we, w)


# 7. the handle's fitted state is untouched
@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_handle_state_unchanged(store):
    M, N, k = 2600, 700, 6
    G = genotypes(M, N, seed=51, special=False)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.upload_genotypes_i8(G)
        e.snp_stats()
        e.rsvd(k, 10, 2, seed=4)
        snap = lambda: [e.scores(), e.scores(f64=True), e.loadings(), e.eigenvalues(), e.transform()] + list(e.get_standardization().values())
        before = snap()
        K = len(e.pca_snp_rows())
        out = e.ld_window(count_windows(K, 50), wmax=50, threshold=0.2, counts=True)
        e.ld_window(count_windows(K, 50, 100, 300), wmax=50, rows=(100, 300))
        after = snap()
        for a, b in zip(before, after):
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
        keep = e.get_standardization()["keep"]
    ref = ref_ld(G, keep, count_windows(K, 50), 50)
    assert np.array_equal(out["r2"], ref[0], equal_nan=True) and np.array_equal(out["counts"], ref[1])


# 8. error codes
def test_errors():
    M, N, w = 700, 300, 20
    G = genotypes(M, N, seed=61, special=False)
    lib = _lib.load()
    r2 = np.zeros((M, w))
    ab = np.zeros((M, 1), np.uint64)
    we = count_windows(M, w)

    def call(e, r0, r1, win, wmax, thr=0.2, o_r2=r2, o_ab=None):
        win = np.ascontiguousarray(win, np.int64)
        return lib.gpca_ld_window(e._h, r0, r1, win.ctypes.data, wmax, thr, None if o_r2 is None else o_r2.ctypes.data, None,
                                  None if o_ab is None else o_ab.ctypes.data)
    with gpca.GpcaEngine() as e:                                  # no genotypes
        assert call(e, 0, 1, we, w) == _lib.GPCA_ERR_STATE
    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(G)
        assert call(e, 0, M, we, w) == _lib.GPCA_ERR_STATE        # no standardisation
        e.snp_stats(gpca.QcConfig.none())
        K = len(e.pca_snp_rows())
        assert K == M
        for r0, r1 in ((-1, M), (10, 3), (0, M + 1)):
            assert call(e, r0, r1, we, w) == _lib.GPCA_ERR_BAD_ARG, (r0, r1)
        assert call(e, 0, M, we, 0) == _lib.GPCA_ERR_BAD_ARG                              # wmax
        assert call(e, 0, M, we, w, o_r2=None) == _lib.GPCA_ERR_BAD_ARG                   # every output NULL
        for thr in (np.nan, np.inf):
            assert call(e, 0, M, we, w, thr=thr, o_ab=ab) == _lib.GPCA_ERR_BAD_ARG        # threshold, read with above
        assert call(e, 0, M, we, w, thr=np.nan) == _lib.GPCA_OK                           # ... and only with above
        for t, v in ((5, 5), (5, 6 + w + 1), (M - 1, M + 1)):                             # win_end below i + 1, past the window, past K
            bad = we.copy(); bad[t] = v
            assert call(e, 0, M, bad, w) == _lib.GPCA_ERR_BAD_ARG, (t, v)
            assert f"row {t}" in lib.gpca_last_error(e._h).decode()
        assert call(e, 0, M, we, 1 << 30) == _lib.GPCA_ERR_OOM                            # 700 x 2^30 slots: refused before any allocation
        assert "device memory" in lib.gpca_last_error(e._h).decode()
        assert call(e, 0, M, we, w) == _lib.GPCA_OK
        st = e.get_standardization()
        e.set_standardization(st["mu"], st["sigma"], np.zeros(M, np.uint8))
        assert call(e, 0, 0, we[:0], w) == _lib.GPCA_ERR_STATE    # K = 0
    Gb = G.copy()
    Gb[17, 40] = 3
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        load(e, Gb)
        assert call(e, 0, M, we, w) == _lib.GPCA_ERR_INVALID_GENOTYPE
        assert "row 17" in lib.gpca_last_error(e._h).decode()
        assert call(e, 100, M, we[100:], w) == _lib.GPCA_OK       # a band that does not read the row
        keep = np.ones(M, np.uint8); keep[17] = 0                 # outside the kept rows: fine
        load(e, Gb, keep)
        assert call(e, 0, M - 1, count_windows(M - 1, w), w) == _lib.GPCA_OK
    with gpca.GpcaEngine() as e:                                  # a streamed handle
        e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), M, N, panel_rows=256, ring_slots=2, fused=False)
        e.snp_stats(gpca.QcConfig.none())
        assert call(e, 0, M, we, w) == _lib.GPCA_ERR_STATE
        assert "panel" in lib.gpca_last_error(e._h).decode()


def test_two_rank_hook_handle_is_refused():
    M, N, w = 600, 200, 20
    G = genotypes(M, N, seed=62, special=False)
    world = 2
    spans = [gpca.shard_rows(M, world, r) for r in range(world)]
    res = [None] * world

    def run(rank):
        a, b_ = spans[rank]
        with gpca.GpcaEngine() as e:
            e.upload_genotypes_i8(G[a:b_].copy())
            e.set_allreduce_hook(lambda buf: None, world, rank, a)
            e.set_standardization(np.ones(b_ - a, np.float32), np.ones(b_ - a, np.float32), np.ones(b_ - a, np.uint8))
            try:
                e.ld_window(count_windows(b_ - a, w), wmax=w)
                res[rank] = "ok"
            except GpcaError as err:
                res[rank] = err
    ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in ts]; [t.join() for t in ts]
    for r in res:
        assert isinstance(r, GpcaError) and r.status == _lib.GPCA_ERR_STATE and "shard" in str(r), r


# 9. a real-LD slice: the golden fixture's .bed rows (64 samples), decoded to A1 dosages
def test_golden_real_ld_slice():
    z = np.load(os.path.join(ROOT, "tests", "golden", "chr22_subset50_120k.npz"))
    n = int(z["n_samples"])
    codes = np.unpackbits(z["bed_rows"][:30000], axis=1, bitorder="little").reshape(30000, -1, 2)
    codes = (codes[..., 0] + 2 * codes[..., 1])[:, :n]                       # .bed: 0 = hom A1, 1 = missing, 2 = het, 3 = hom A2
    G = np.ascontiguousarray(np.array([2, -127, 1, 0], np.int8)[codes])
    keep = z["keep"][:30000].astype(np.uint8)
    K = int(keep.sum())
    assert K > 1000
    for store in ("int8", "2bit"):
        with gpca.GpcaEngine(storage=STORES[store]) as e:
            load(e, G, keep)
            for w in (50, 200):
                out = check(e, G, keep, count_windows(K, w), w)
            with np.errstate(invalid="ignore"):
                assert (out["r2"] > 0.8).sum() > 1000              # real LD: many tightly linked neighbours


# 10. end to end: the Python command line with --gpca-indep-pairwise on a fileset with runs of correlated SNPs on two chromosomes
def test_cli_indep_pairwise_end_to_end(tmp_path):
    from genomic_pca_amd.cli import main
    rng = np.random.default_rng(71)
    M, N = 2400, 300
    p = rng.uniform(0.1, 0.5, size=(M, 1))
    G = (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)
    for i in range(1, M):                                           # runs of 12 correlated SNPs
        if i % 12:
            cp = rng.random(N) < 0.85
            G[i, cp] = G[i - 1, cp]
    # missing calls only where the call-rate filter drops the row: the PCA refuses a kept SNP with a missing call (as the reference does)
    G[200:230][rng.random((30, N)) < 0.1] = -127
    G[100] = 0                                                      # monomorphic: dropped by QC
    chrom = ["1"] * 1300 + ["2"] * 1100
    pos = list(range(1000, 1000 + 1300 * 100, 100)) + list(range(500, 500 + 1100 * 100, 100))
    ids = [f"rs{i}" for i in range(M)]
    pre = str(tmp_path / "in")
    gio.write_plink(pre, G, [f"s{i}" for i in range(N)], ids, chrom, pos)
    ld = tmp_path / "ld.txt"
    ld.write_text("1 1 100000\n1 100501 200000\n2 1 60000\n2 60001 200000\n")      # a gap on chromosome 1 leaves QC-passing SNPs out
    out = str(tmp_path / "o" / "P")
    args = ["--eigensnp", "--bed-file", pre + ".bed", "--ld-block-file", str(ld), "--eigensnp-k-global", "3", "--eigensnp-max-hwe-p", "1.0",
            "--gpca-storage", "int8", "--gpca-indep-pairwise", "50", "0.2", "--out", out]
    assert main(args) == 0
    pin = open(out + ".prune.in").read().split("\n")
    pout = open(out + ".prune.out").read().split("\n")
    assert pin[-1] == "" and pout[-1] == ""
    pin, pout = pin[:-1], pout[:-1]

    # the QC-and-block-kept rows, from the same library calls the command line makes
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        e.upload_genotypes_i8(G)
        st = e.snp_stats(gpca.QcConfig(0.98, 0.01, 1.0))
        counts, _ = e.snp_qc_detail()
    keep, _ = gio.map_snps_to_ld_blocks(gio.parse_ld_block_file(str(ld)), chrom, pos, st["keep"])
    rows = np.flatnonzero(keep)
    assert not keep[100] and not keep[200:230].any() and 0 < len(rows) < M - 1
    assert sorted(pin + pout, key=lambda s: int(s[2:])) == [ids[r] for r in rows]
    assert pin == sorted(pin, key=lambda s: int(s[2:])) and pout == sorted(pout, key=lambda s: int(s[2:]))   # .bim order

    # the in-set is io.ld_prune on ref_ld's r2; no surviving in-window pair is above 0.2 by ref_ld
    K = len(rows)
    we = gio.ld_windows([chrom[r] for r in rows], np.asarray(pos)[rows], "50")
    r2, _ = ref_ld(G, keep, we, 49)
    with np.errstate(invalid="ignore"):
        hot = r2 > 0.2
    above = np.packbits(np.pad(hot, ((0, 0), (0, 64 - 49))), axis=1, bitorder="little").view(np.uint64)
    c = counts[rows]
    inset = gio.ld_prune(we, above, gio.maf_from_qc_detail(c[:, 0], c[:, 2], c[:, 3]))
    assert pin == [ids[r] for r in rows[inset]]
    assert 0.05 * K < inset.sum() < 0.6 * K                         # the runs were thinned, not wiped out
    surv = np.flatnonzero(inset)
    for i in surv:
        js = np.arange(i + 1, we[i])
        assert not (hot[i, :len(js)] & inset[js]).any()
    load_ids = [ln.split("\t")[0] for ln in open(out + ".eigensnp.loadings.tsv").read().split("\n")[1:-1]]
    assert load_ids == pin
