"""gpca_ld_score (include/gpca.h section a19; k_ld_score in ld.hip) held to two exact integer models.  Every comparison is
np.array_equal: there is no tolerance anywhere.

(A) ``model_a``: from the genotypes alone.  The six counts of every pair come from ``ld_model`` of test_gpu_ld_exact.py (numpy, int64),
    r2 from its ``finish`` (the f64 expression of k_ld_finish), then ``reduce_pairs``: a pair is skipped when r2 is NaN (vx <= 0 or
    vy <= 0) or n <= 2; otherwise v = r2 - (1.0 - r2) / (n - 2.0) (unbiased) or r2, q = np.rint(v * 2.0**40) as int64 (numpy rounds half
    to even and contracts nothing), added at the row and at the partner, with 1 added to the partner counts at the same two places.
(B) ``model_b``: ``reduce_pairs`` on the r2 and counts that e.ld_window returns for the same band -- the new kernel tied to the bits
    of the existing one.

Every case lies in the exact regime of test_gpu_ld_exact.py (the largest sample count is 4 097: every product is below 2^27), so the
three differences are exact with or without a fused multiply-add.

Shapes: samples in {1, 2, 3, 17, 64, 129, 257, 4097} (N <= 2 gives all zeros; 4 097 samples with 5 rows puts k_ld on its sample split);
kept rows in {1, 2, 63, 64, 65, 129, 200} (the 64-row tile of k_ld_score on both sides) and 600 (a window wider than the 256-slot tile:
w in {255, 256, 257, 300, 513}, two and three slot tiles); wmax in {1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300}; uniform
windows, ragged ones with two chromosome ends (empty windows in the middle), windows clipped at K, wmax above the widest window; the keep
masks of _edges.py."""
import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from genomic_pca_amd import io as gio
from genomic_pca_amd._lib import GpcaError
from _edges import edge_keeps
from test_gpu_ld_exact import MISSING, ld_model

TWO40 = 2 ** 40
WMAX = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300]
STORES = {"int8": _lib.STORE_INT8, "2bit": _lib.STORE_2BIT}


# ---------------------------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------------------------
def reduce_pairs(r2, counts, inwin, span, unbiased):
    """(score int64 [span], partners int32 [span]) of a band from r2 [rows][wmax] f64, counts [rows][wmax][6] and the window mask"""
    n = counts[..., 0].astype(np.float64)
    ok = inwin & ~np.isnan(r2) & (n > 2.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = r2 - (1.0 - r2) / (n - 2.0) if unbiased else r2
        q = np.where(ok, np.rint(np.where(ok, v, 0.0) * 2.0 ** 40), 0.0).astype(np.int64)
    t, d = np.nonzero(ok)
    score = np.zeros(span, np.int64)
    part = np.zeros(span, np.int32)
    np.add.at(score, t, q[t, d]); np.add.at(score, t + 1 + d, q[t, d])
    np.add.at(part, t, 1); np.add.at(part, t + 1 + d, 1)
    return score, part


def span_of(K, r0, r1, wmax):
    return min(K, r1 + wmax) - r0 if r1 > r0 else 0


def model_a(G, keep, we, wmax, r0, r1, unbiased):
    K = int(np.asarray(keep).sum())
    if r1 == r0:
        return np.zeros(0, np.int64), np.zeros(0, np.int32)
    m = ld_model(G, keep, we, wmax, r0, r1)
    return reduce_pairs(m.r2, m.counts, m.inwin, span_of(K, r0, r1, wmax), unbiased)


def model_b(e, K, we, wmax, r0, r1, unbiased):
    out = e.ld_window(we, wmax=wmax, rows=(r0, r1), counts=True)
    inwin = (np.arange(r0, r1)[:, None] + 1 + np.arange(wmax)[None, :]) < np.asarray(we)[:, None]
    return reduce_pairs(out["r2"], out["counts"], inwin, span_of(K, r0, r1, wmax), unbiased)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def genotypes(M, N, seed, miss=0.02):
    """LD by construction: a row copies the row before it on 70 % of the samples"""
    rng = np.random.default_rng([41, M, N, seed])
    p = rng.uniform(0.05, 0.5, size=(M, 1))
    G = (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)
    cp = rng.random((M, N)) < 0.7
    for i in range(1, M):
        if i % 7:
            G[i, cp[i]] = G[i - 1, cp[i]]
    if miss:
        G[rng.random((M, N)) < miss] = MISSING
    return G


def scattered_keep(K, seed=0):
    M = K + 40
    keep = np.zeros(M, np.uint8)
    keep[np.random.default_rng([43, K, seed]).choice(M, K, replace=False)] = 1
    return keep


def uniform_windows(K, w):
    return np.minimum(np.arange(K, dtype=np.int64) + 1 + w, K)


def ragged_windows(K, w, seed=0):
    """random widths up to w, two chromosome ends inside (rows with empty windows in the middle) and the end of the rows"""
    rng = np.random.default_rng([47, K, w, seed])
    i = np.arange(K, dtype=np.int64)
    width = rng.integers(0, w + 1, size=K)
    width[rng.integers(0, K)] = w
    ends = np.array(sorted({K // 3, 2 * K // 3, K}), np.int64)
    ends = ends[ends > 0]
    return np.minimum(i + 1 + width, ends[np.searchsorted(ends, i, side="right")])


def open_handle(e, G, keep):
    M = G.shape[0]
    e.upload_genotypes_i8(G)
    e.snp_stats(gpca.QcConfig.none())
    e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), keep)
    assert np.array_equal(e.pca_snp_rows(), np.flatnonzero(keep))


def check(e, G, keep, we, wmax, band=None, flags=(True, False), tie=True):
    """the device's score and partners of one band against (A) and, with tie, (B), in the flag modes asked for; returns the outputs"""
    K = int(keep.sum())
    r0, r1 = (0, K) if band is None else band
    we = np.asarray(we, np.int64)[r0:r1] if len(we) == K else np.asarray(we, np.int64)
    outs = []
    for unb in flags:
        out = e.ld_score(we, wmax=wmax, rows=(r0, r1), unbiased=unb, partners=True)
        sa, pa = model_a(G, keep, we, wmax, r0, r1, unb)
        assert out["score"].dtype == np.int64 and out["partners"].dtype == np.int32
        assert out["score"].shape == sa.shape and out["partners"].shape == pa.shape, (out["score"].shape, sa.shape)
        assert np.array_equal(out["partners"], pa), ("partners (A)", K, wmax, band, unb)
        assert np.array_equal(out["score"], sa), ("score (A)", K, wmax, band, unb)
        if tie and r1 > r0:
            sb, pb = model_b(e, K, we, wmax, r0, r1, unb)
            assert np.array_equal(out["score"], sb) and np.array_equal(out["partners"], pb), ("(B)", K, wmax, band, unb)
        outs.append(out)
    if len(flags) == 2:
        assert (outs[1]["score"] >= outs[0]["score"]).all()                  # raw >= unbiased, element-wise
        assert np.array_equal(outs[0]["partners"], outs[1]["partners"])
    return outs


# ---------------------------------------------------------------------------------------------------------------------------------
# device tests
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2, 3, 17, 64, 129, 257, 4097])
def test_sample_counts_equal_the_models(N):
    K = 5 if N == 4097 else 200
    keep = scattered_keep(K)
    G = genotypes(keep.size, N, seed=1)
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        open_handle(e, G, keep)
        for w, wmax in ((4, 4),) if K == 5 else ((1, 1), (65, 65), (65, 68), (199, 300)):
            outs = check(e, G, keep, uniform_windows(K, w), wmax)
            if N <= 2:
                assert not outs[0]["score"].any() and not outs[0]["partners"].any() and not outs[1]["score"].any()
            elif N >= 17:
                assert outs[0]["partners"].any() and outs[1]["score"].any()
        if K > 5:
            check(e, G, keep, ragged_windows(K, 70), 73)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 129, 200])
@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_kept_rows_and_window_widths_equal_the_models(store, K):
    keep = scattered_keep(K)
    G = genotypes(keep.size, 129, seed=2)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        open_handle(e, G, keep)
        for wmax in WMAX:                                                    # uniform windows clipped at K, wmax = w
            check(e, G, keep, uniform_windows(K, wmax), wmax, tie=wmax in (1, 64, 65, 257))
        check(e, G, keep, uniform_windows(K, 33), 40)                        # wmax above the widest window
        check(e, G, keep, ragged_windows(K, 70), 73)


@pytest.mark.gpu
@pytest.mark.parametrize("w", [255, 256, 257, 300, 513])
def test_windows_wider_than_the_slot_tile_equal_the_models(w):
    K = 600
    keep = scattered_keep(K)
    G = genotypes(keep.size, 64, seed=3)
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        open_handle(e, G, keep)
        check(e, G, keep, uniform_windows(K, w), w)
        check(e, G, keep, ragged_windows(K, w), w + 3, flags=(True,))
        check(e, G, keep, uniform_windows(K, w), w, band=(63, 300), flags=(True,))     # row0 off the tile, windows past row1


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, _ in edge_keeps(170)])
def test_edge_keep_masks_equal_the_models(name):
    keep = dict(edge_keeps(170))[name]
    K = int(keep.sum())
    G = genotypes(170, 129, seed=4)
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        open_handle(e, G, keep)
        for w in (1, 65, 200):
            check(e, G, keep, uniform_windows(K, w), w)
        check(e, G, keep, ragged_windows(K, 70), 73)


@pytest.mark.gpu
def test_every_split_into_two_bands_adds_up_to_the_full_call():
    K, rows, wmax = 110, 70, 33
    keep = scattered_keep(K)
    G = genotypes(keep.size, 129, seed=5)
    we = ragged_windows(K, wmax)
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        open_handle(e, G, keep)
        full = check(e, G, keep, we[:rows], wmax, band=(0, rows), flags=(True,))[0]
        span = full["score"].size
        assert span == rows + wmax and full["score"][rows:].any()            # the entries past row1 are there and in use
        for s in range(0, rows + 1):
            bands = []
            for r0, r1 in ((0, s), (s, rows)):
                o = e.ld_score(we[r0:r1], wmax=wmax, rows=(r0, r1), partners=True)
                assert o["score"].size == span_of(K, r0, r1, wmax)
                bands.append(((r0, r1), o["score"], o["partners"]))
            acc, part = gio.ld_score_sum(K, bands)
            assert np.array_equal(acc[:span], full["score"]) and not acc[span:].any(), s
            assert np.array_equal(part[:span], full["partners"]) and not part[span:].any(), s


@pytest.mark.gpu
@pytest.mark.parametrize("miss", ["none", "2 %", "special rows"])
def test_missing_calls_equal_the_models(miss):
    K, N = 130, 129
    keep = scattered_keep(K)
    G = genotypes(keep.size, N, seed=6, miss=0.02 if miss == "2 %" else 0.0)
    kr = np.flatnonzero(keep)
    if miss == "special rows":
        G[kr[10], 3:] = MISSING                                              # observed at 3 samples only: n <= 3 with every partner
        G[kr[11], :2] = MISSING; G[kr[11], 3:] = MISSING                     # ... and its neighbour at one of them: n = 1, skipped
        a, b = kr[40], kr[41]                                                # a pair whose jointly observed samples have no variance
        G[a] = 0; G[a, :40] = 1; G[a, 40:] = np.where(np.arange(N - 40) % 2, MISSING, 0)
        G[b, :40] = MISSING; G[b, 40:] = (np.arange(N - 40) % 3).astype(np.int8)
        G[kr[70]] = 2                                                        # a monomorphic kept row
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        open_handle(e, G, keep)
        outs = check(e, G, keep, uniform_windows(K, 65), 65)
        check(e, G, keep, uniform_windows(K, 65), 65, band=(5, 90))
        if miss == "special rows":
            m = ld_model(G, keep, uniform_windows(K, 65), 65)
            assert m.counts[40, 0, 0] > 2 and np.isnan(m.r2[40, 0])          # jointly observed, no variance there: skipped, not counted
            assert (m.counts[10, :, 0] <= 3).all() and m.counts[10, 0, 0] == 1
            assert outs[0]["partners"][70] == 0 and outs[0]["score"][70] == 0 and outs[1]["score"][70] == 0


@pytest.mark.gpu
def test_fixtures_with_known_answers():
    N = 50
    rng = np.random.default_rng(53)
    g = rng.integers(0, 3, size=N).astype(np.int8)
    g[:3] = (0, 1, 2)
    keep5 = np.ones(5, np.uint8)
    for G in (np.tile(g, (5, 1)), np.stack([g, 2 - g, g, 2 - g, g]).astype(np.int8)):     # identical rows; complementary rows
        with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
            open_handle(e, G, keep5)
            for unb in (True, False):
                out = e.ld_score(uniform_windows(5, 4), unbiased=unb, partners=True)
                assert np.array_equal(out["score"], np.full(5, 4 * TWO40, np.int64)) and np.array_equal(out["partners"], np.full(5, 4, np.int32))
            l2 = gpca.GpcaEngine.ld_score_total(out["score"])
            assert np.array_equal(l2, np.full(5, 5.0))
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:                      # two complementary rows alone
        open_handle(e, np.stack([g, 2 - g]).astype(np.int8), np.ones(2, np.uint8))
        out = e.ld_score(uniform_windows(2, 1), partners=True)
        assert out["score"].tolist() == [TWO40, TWO40] and out["partners"].tolist() == [1, 1]


@pytest.mark.gpu
def test_storage_and_precision_give_the_same_bits():
    K = 200
    keep = scattered_keep(K)
    G = genotypes(keep.size, 1100, seed=7)                                   # (2-bit rows pad to 1 024 samples: one past it)
    we = ragged_windows(K, 70)
    got = []
    for prec, store in ((_lib.PREC_I8_EXACT, "int8"), (_lib.PREC_I8_EXACT, "2bit"), (_lib.PREC_F32_MFMA, "int8")):
        with gpca.GpcaEngine(precision=prec, storage=STORES[store]) as e:
            open_handle(e, G, keep)
            got.append(check(e, G, keep, we, 73, tie=False)[0])
    for o in got[1:]:
        assert np.array_equal(o["score"], got[0]["score"]) and np.array_equal(o["partners"], got[0]["partners"])


@pytest.mark.gpu
def test_errors():
    M, N, w = 300, 100, 20
    G = genotypes(M, N, seed=8)
    lib = _lib.load()
    score = np.zeros(M, np.int64)
    part = np.zeros(M, np.int32)
    we = uniform_windows(M, w)

    def call(e, r0, r1, win, wmax, flags=1, o_score=score, o_part=part):
        win = np.ascontiguousarray(win, np.int64)
        return lib.gpca_ld_score(e._h, r0, r1, win.ctypes.data, wmax, flags, None if o_score is None else o_score.ctypes.data,
                                 None if o_part is None else o_part.ctypes.data)
    with gpca.GpcaEngine() as e:                                             # no genotypes
        assert call(e, 0, 1, we, w) == _lib.GPCA_ERR_STATE
    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(G)
        assert call(e, 0, M, we, w) == _lib.GPCA_ERR_STATE                   # no standardisation
        assert "standardisation" in lib.gpca_last_error(e._h).decode()
        e.snp_stats(gpca.QcConfig.none())
        assert len(e.pca_snp_rows()) == M
        for r0, r1 in ((-1, M), (10, 3), (0, M + 1)):
            assert call(e, r0, r1, we, w) == _lib.GPCA_ERR_BAD_ARG, (r0, r1)
        assert call(e, 0, M, we, 0) == _lib.GPCA_ERR_BAD_ARG                 # wmax 0
        assert call(e, 0, M, we, (1 << 20) + 1) == _lib.GPCA_ERR_BAD_ARG and "2^20" in lib.gpca_last_error(e._h).decode()
        assert call(e, 0, M, we, w, o_score=None) == _lib.GPCA_ERR_BAD_ARG
        assert call(e, 0, M, we, w, flags=2) == _lib.GPCA_ERR_BAD_ARG
        for t, v in ((5, 5), (5, 6 + w + 1), (M - 1, M + 1)):                # win_end below i + 1, past the window, past K
            bad = we.copy(); bad[t] = v
            assert call(e, 0, M, bad, w) == _lib.GPCA_ERR_BAD_ARG, (t, v)
            assert f"row {t}" in lib.gpca_last_error(e._h).decode()
        score[:] = 7; part[:] = 7
        assert call(e, 40, 40, we[:0], w) == _lib.GPCA_OK and (score == 7).all() and (part == 7).all()     # rows = 0 writes nothing
        assert call(e, 0, M, we, w, o_part=None) == _lib.GPCA_OK and (part == 7).all()                      # partners = NULL
        want = e.ld_score(we, wmax=w, partners=True)
        assert np.array_equal(score, want["score"])
        st = e.get_standardization()
        e.set_standardization(st["mu"], st["sigma"], np.zeros(M, np.uint8))
        assert call(e, 0, 0, we[:0], w) == _lib.GPCA_ERR_STATE               # K = 0
        assert "keep mask" in lib.gpca_last_error(e._h).decode()
    Gb = G.copy()
    Gb[17, N - 1] = 3                                                        # an invalid byte below N
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        open_handle(e, Gb, np.ones(M, np.uint8))
        assert call(e, 0, M, we, w) == _lib.GPCA_ERR_INVALID_GENOTYPE and "row 17 " in lib.gpca_last_error(e._h).decode()
        assert call(e, 100, M, we[100:], w) == _lib.GPCA_OK                  # a band that does not read the row
        with pytest.raises(GpcaError):
            e.ld_score(we, wmax=w)
    with gpca.GpcaEngine() as e:                                             # a streamed handle
        e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), M, N, panel_rows=256, ring_slots=2, fused=False)
        e.snp_stats(gpca.QcConfig.none())
        assert call(e, 0, M, we, w) == _lib.GPCA_ERR_STATE and "panel" in lib.gpca_last_error(e._h).decode()


def test_host_total_on_a_hand_made_vector():
    acc = np.array([0, TWO40, -TWO40 // 2, 3 * TWO40 + 1, 1], np.int64)
    l2 = gpca.GpcaEngine.ld_score_total(acc)
    assert l2.tolist() == [1.0, 2.0, 0.5, 4.0 + 2.0 ** -40, 1.0 + 2.0 ** -40]
    assert gpca.GpcaEngine.ld_score_total(np.zeros(0, np.int64)).shape == (0,)
