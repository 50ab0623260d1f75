"""gpca_f2_blocks (f2_blocks.hip, gpca_f2_blocks.cpp; include/gpca.h section a23) through the C ABI against a numpy model.

The sums are exact integers, so every comparison is ``array_equal``.  The model (``model_f2``): the counts of
``test_gpu_group_counts.model``, then a23's f64 chain in numpy, one ufunc per operation (no fused multiply-add), ``np.rint`` (half to
even) and ``np.add.at`` over (block, pair).

Shapes: the sample axis belongs to the group-counts tests, so three sample counts (33, 257, 1025) are enough.  Rows: one, and each of
the kernel's two extents -- the LDS tile of 32 rows and the workgroup's run of 256 (kFbTile, kFbRun in plan_math.h) -- with one less
and one more.  Groups: 2, 3, 23 and 24 (253 and 276 pairs straddle the 256 threads), 32, 33, 63 and 64 (2 016 pairs fill the eighth
register slot; 33 is the first count with two one-hot column blocks).  Block patterns over three workgroups: one block, every row its
own, a boundary at every tile and workgroup edge and one row either side, -1 rows and a call of nothing else, non-monotone ids, more
blocks than ids.  Data: an empty group, a group whose calls are all missing on some rows, a group of one sample (n - 1 = 1), groups
drawn from one population (negative q; the model is asserted to have them).  Invariance: the keep masks of tests/_edges.py, every
split of a 70-row call into two bands, both storages and an f32-precision handle, counts=True against group_counts.  a23's error
list, and the timing record."""
import ctypes

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from genomic_pca_amd._lib import GpcaError

from _edges import edge_keeps
from test_gpu_group_counts import STORES, load, make, model

pytestmark = pytest.mark.gpu

FB_TILE, FB_RUN = 32, 256        # kFbTile, kFbRun (plan_math.h)
MS = [1, FB_TILE - 1, FB_TILE, FB_TILE + 1, FB_RUN - 1, FB_RUN, FB_RUN + 1]
PS = [2, 3, 23, 24, 32, 33, 63, 64]


def pair_index(P):
    """(I, J): the groups of pair i (i - 1) / 2 + j, j < i"""
    I = np.array([i for i in range(1, P) for j in range(i)], np.int64)
    J = np.array([j for i in range(1, P) for j in range(i)], np.int64)
    assert np.array_equal(I * (I - 1) // 2 + J, np.arange(P * (P - 1) // 2))
    return I, J


def model_f2(counts, block, B, want_q=False):
    """(acc, cnt) int64 [B][pairs] from counts uint32 [rows][P][3] and block [rows]"""
    P = counts.shape[1]
    I, J = pair_index(P)
    c = counts.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = 2.0 * c[..., 0]
        p = (c[..., 1] + 2.0 * c[..., 2]) / n
        h = (p * (1.0 - p)) / (n - 1.0)
        d = p[:, I] - p[:, J]
        v = (d * d - h[:, I]) - h[:, J]
        ok = (counts[:, I, 0] >= 1) & (counts[:, J, 0] >= 1) & (np.asarray(block) >= 0)[:, None]
        q = np.where(ok, np.rint(np.where(ok, v, 0.0) * 2.0 ** 40), 0.0).astype(np.int64)
    acc = np.zeros((B, len(I)), np.int64)
    cnt = np.zeros((B, len(I)), np.int64)
    r, k = np.nonzero(ok)
    np.add.at(acc, (np.asarray(block)[r], k), q[r, k])
    np.add.at(cnt, (np.asarray(block)[r], k), 1)
    return (acc, cnt, q, ok) if want_q else (acc, cnt)


def runs(M, length, start=0):
    """block ids in runs of `length` rows"""
    return ((np.arange(M) + start) // length).astype(np.int32)


def check(e, G, group, P, block, B, keep=None, rows=None):
    got = e.f2_blocks(group, block, P, B, rows=rows)
    cm = model(G, group, P, keep)
    if rows is not None:
        cm = cm[rows[0]:rows[1]]
    want = model_f2(cm, block, B)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int64 and got[0].shape == want[0].shape == got[1].shape
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])
    return want


@pytest.mark.parametrize("store", sorted(STORES))
def test_row_counts(store):
    N, P = 257, 5
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        for i, M in enumerate(MS):
            G, group = make(M, N, P, seed=1100 + i)
            load(e, G)
            check(e, G, group, P, runs(M, 7), (M + 6) // 7)
            check(e, G, group, P, np.zeros(M, np.int32), 1)


@pytest.mark.parametrize("store", sorted(STORES))
def test_group_counts_P(store):
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        for i, P in enumerate(PS):
            N = (33, 257, 1025)[i % 3] if P <= 33 else 257
            M = FB_TILE + 38
            G, group = make(M, N, P, seed=1200 + i)
            group[:min(P, N)] = np.arange(min(P, N))
            load(e, G)
            acc, cnt = check(e, G, group, P, runs(M, 9), (M + 8) // 9)
            assert acc.shape[1] == P * (P - 1) // 2
            if P <= N:
                assert cnt[:, -1].sum() > 0                       # the last pair of the last slot is live


def boundary_blocks(M):
    """a block boundary at every tile and workgroup edge of three workgroups, and one row either side of each"""
    cuts = set()
    for edge in list(range(FB_TILE, M, FB_TILE)):
        if edge % FB_RUN == 0 or edge in (FB_TILE, FB_RUN - FB_TILE, FB_RUN + FB_TILE):
            cuts.update((edge - 1, edge, edge + 1))
    block = np.zeros(M, np.int32)
    for c in sorted(x for x in cuts if 0 < x < M):
        block[c:] += 1
    return block


def test_block_patterns():
    M, N, P = 2 * FB_RUN + 88, 33, 6
    G, group = make(M, N, P, seed=1300)
    rng = np.random.default_rng(1301)
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        load(e, G)
        check(e, G, group, P, np.zeros(M, np.int32), 1)                                   # one block
        check(e, G, group, P, np.arange(M, dtype=np.int32), M)                            # every row its own block
        bb = boundary_blocks(M)
        assert bb[FB_RUN - 1] != bb[FB_RUN] != bb[FB_RUN + 1] and bb[FB_TILE - 1] != bb[FB_TILE] and bb[2 * FB_RUN - 2] != bb[2 * FB_RUN - 1]
        check(e, G, group, P, bb, int(bb.max()) + 1)
        some = runs(M, 40)
        some[rng.random(M) < 0.3] = -1                                                    # rows that enter nothing
        some[FB_RUN - 3:FB_RUN + 3] = -1
        want = check(e, G, group, P, some, int(some.max()) + 1)
        assert want[1].sum() < model_f2(model(G, group, P), runs(M, 40), int(some.max()) + 1)[1].sum()
        none = np.full(M, -1, np.int32)
        acc, cnt = e.f2_blocks(group, none, P, 4)                                         # a call of nothing but -1
        assert acc.shape == (4, 15) and not acc.any() and not cnt.any()
        shuffled = rng.integers(0, 5, M).astype(np.int32)                                 # non-monotone ids
        check(e, G, group, P, shuffled, 5)
        down = (M - 1 - np.arange(M)) // 50
        check(e, G, group, P, down.astype(np.int32), int(down.max()) + 1)
        want = check(e, G, group, P, runs(M, 100), 40)                                    # B larger than the ids used
        assert not want[1][6:].any()
        acc, cnt = e.f2_blocks(group, runs(M, 100), P)                                    # n_blocks defaults to the largest id + 1
        assert acc.shape[0] == 6 and np.array_equal(acc, want[0][:6]) and np.array_equal(cnt, want[1][:6])


@pytest.mark.parametrize("store", sorted(STORES))
def test_data_edges(store):
    M, N, P = FB_TILE + 9, 257, 6
    G, group = make(M, N, P, seed=1400)
    group = np.where(group == 2, 3, group).astype(np.int32)          # group 2 is empty
    one = np.flatnonzero(group == 4)
    group[one[1:]] = 5                                               # group 4 holds one sample: n - 1 = 1 where it has a call
    G[3:9, group == 1] = -127                                        # group 1 has no call on rows 3 .. 8
    G[12, one[0]] = -127                                             # ... and the single sample none on row 12
    cm = model(G, group, P)
    assert not cm[:, 2].any() and cm[:, 4, 0].max() == 1 and cm[12, 4, 0] == 0 and not cm[3:9, 1, 0].any() and cm[9, 1, 0] > 0
    block = runs(M, 5)
    B = int(block.max()) + 1
    acc, cnt, q, ok = model_f2(cm, block, B, want_q=True)
    assert (q[ok] < 0).any() and (q[ok] > 0).any()                   # the groups are one population: negative f2 occur
    I, J = pair_index(P)
    assert not cnt[:, (I == 2) | (J == 2)].any() and cnt[:, (I == 5) & (J == 3)].sum() == M
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        load(e, G)
        got = e.f2_blocks(group, block, P, B)
        assert np.array_equal(got[0], acc) and np.array_equal(got[1], cnt)


def test_keep_masks():
    M, N, P = FB_RUN + 1, 257, 4
    G, group = make(M, N, P, seed=1500)
    with gpca.GpcaEngine(storage=_lib.STORE_2BIT) as e:
        for name, keep in edge_keeps(M):
            load(e, G, keep)
            K = int(keep.sum())
            check(e, G, group, P, runs(K, 33), (K + 32) // 33, keep=keep)


@pytest.mark.parametrize("store", sorted(STORES))
def test_every_band_split_of_a_70_row_call(store):
    P = 33
    G, group = make(70, 257, P, seed=1600)
    block = runs(70, 11, start=4)
    B = int(block.max()) + 1
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        load(e, G)
        full = check(e, G, group, P, block, B)
        for s in range(71):
            a = e.f2_blocks(group, block[:s], P, B, rows=(0, s))
            b = e.f2_blocks(group, block[s:], P, B, rows=(s, 70))
            assert np.array_equal(a[0] + b[0], full[0]) and np.array_equal(a[1] + b[1], full[1]), s


def test_storages_precisions_and_counts_agree():
    M, N, P = FB_RUN + 5, 1025, 40
    G, group = make(M, N, P, seed=1700)
    block = runs(M, 60)
    B = int(block.max()) + 1
    cm = model(G, group, P)
    want = model_f2(cm, block, B)
    for store, prec in (("int8", _lib.PREC_I8_EXACT), ("2bit", _lib.PREC_I8_EXACT), ("int8", _lib.PREC_F32_MFMA)):
        with gpca.GpcaEngine(precision=prec, storage=STORES[store]) as e:
            load(e, G)
            acc, cnt, counts = e.f2_blocks(group, block, P, B, counts=True)
            assert np.array_equal(acc, want[0]) and np.array_equal(cnt, want[1]), (store, prec)
            assert counts.dtype == np.uint32 and np.array_equal(counts, cm) and np.array_equal(counts, e.group_counts(group, P))
            a2, c2, k2 = e.f2_blocks(group, block[10:50], P, B, rows=(10, 50), counts=True)
            assert np.array_equal(k2, cm[10:50]) and np.array_equal(a2, model_f2(cm[10:50], block[10:50], B)[0])


def test_error_paths():
    N, M, P, B = 130, 40, 3, 4
    G, group = make(M, N, P, seed=1800)
    block = runs(M, 10)
    lib = _lib.load()
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        e.upload_genotypes_i8(G)
        acc, cnt = np.ones((B, 3), np.int64), np.ones((B, 3), np.int64)

        def raw(g, p, r0, r1, blk, b, a, c, k=None):
            rc = lib.gpca_f2_blocks(e._h, vp(g), p, r0, r1, vp(blk), b, vp(a), vp(c), vp(k))
            return rc, lib.gpca_last_error(e._h).decode()
        got = raw(group, P, 0, M, block, B, acc, cnt)                                    # no standardisation
        assert got[0] == _lib.GPCA_ERR_STATE and "gpca_f2_blocks" in got[1] and "standardisation" in got[1], got
        load(e, G)
        cm = model(G, group, P)
        want = model_f2(cm, block, B)
        assert raw(group, P, 0, M, block, B, acc, cnt)[0] == _lib.GPCA_OK
        assert np.array_equal(acc, want[0]) and np.array_equal(cnt, want[1])             # written, not added to
        big = group.copy(); big[7] = P
        lo, hi = block.copy(), block.copy()
        lo[5] = -2; hi[6] = B
        for got, word in ((raw(None, P, 0, M, block, B, acc, cnt), "group"), (raw(group, P, 0, M, None, B, acc, cnt), "block"),
                          (raw(group, P, 0, M, block, B, None, cnt), "acc"), (raw(group, P, 0, M, block, B, acc, None), "cnt"),
                          (raw(group, P, 0, M, block, 0, acc, cnt), "B must"), (raw(group, P, 0, M, block, -3, acc, cnt), "B must"),
                          (raw(group, 1, 0, M, block, B, acc, cnt), "P must"), (raw(group, 0, 0, M, block, B, acc, cnt), "P must"),
                          (raw(group, 65, 0, M, block, B, acc, cnt), "P must"), (raw(big, P, 0, M, block, B, acc, cnt), "group[7]"),
                          (raw(group, P, 0, M, lo, B, acc, cnt), "block[5]"), (raw(group, P, 0, M, hi, B, acc, cnt), "block[6]"),
                          (raw(group, P, 2, M, hi[2:], B, acc, cnt), "kept row 6"),
                          (raw(group, P, -1, M, block, B, acc, cnt), "rows"), (raw(group, P, 3, 2, block, B, acc, cnt), "rows"),
                          (raw(group, P, 0, M + 1, block, B, acc, cnt), "rows")):
            assert got[0] == _lib.GPCA_ERR_BAD_ARG and word in got[1] and "gpca_f2_blocks" in got[1], got
        acc[:], cnt[:] = 1, 1
        assert raw(group, P, 5, 5, block, B, acc, cnt)[0] == _lib.GPCA_OK and not acc.any() and not cnt.any()   # an empty band: zeros
        # an invalid byte on a sample with label -1, and on a labelled one
        for lab in (-1, 1):
            Gb = G.copy(); Gb[17, 9] = 3
            gb = group.copy(); gb[9] = lab
            load(e, Gb)
            with pytest.raises(GpcaError) as ei:
                e.f2_blocks(gb, block, P, B)
            assert ei.value.status == _lib.GPCA_ERR_INVALID_GENOTYPE and "row 17" in str(ei.value)
            got = e.f2_blocks(gb, block[:17], P, B, rows=(0, 17))                        # a band that does not read the row
            assert np.array_equal(got[0], model_f2(model(Gb[:17], gb, P), block[:17], B)[0])
        # K = 0: an empty keep mask
        e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.zeros(M, np.uint8))
        with pytest.raises(GpcaError) as ei:
            e.f2_blocks(group, block[:0], P, B)
        assert ei.value.status == _lib.GPCA_ERR_STATE and "no kept row" in str(ei.value)
    # (GPCA_ERR_OOM needs sums or counts beyond the free memory of the card: no shape a quick test can hold reaches it)
    with gpca.GpcaEngine() as e:                                                         # a streamed handle
        e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), M, N, panel_rows=256, ring_slots=2, fused=False)
        e.snp_stats(gpca.QcConfig.none())
        with pytest.raises(GpcaError) as ei:
            e.f2_blocks(group, block, P, B)
        assert ei.value.status == _lib.GPCA_ERR_STATE and "panel" in str(ei.value)
    with gpca.GpcaEngine() as e:                                                         # a hooked (row-sharded) handle
        e.upload_genotypes_i8(G[:20].copy())
        e.set_allreduce_hook(lambda buf: None, 2, 0, 0)
        e.set_standardization(np.ones(20, np.float32), np.ones(20, np.float32), np.ones(20, np.uint8))
        with pytest.raises(GpcaError) as ei:
            e.f2_blocks(group, block[:20], P, B)
        assert ei.value.status == _lib.GPCA_ERR_STATE and "shard" in str(ei.value)


def test_a_band_above_2_to_21_rows_is_refused():
    M, N = (1 << 21) + 1, 4
    with gpca.GpcaEngine(storage=_lib.STORE_2BIT) as e:
        e.synth_genotypes(M, N, 1, np.full((M, 1), 1 << 31, np.uint32))
        e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.ones(M, np.uint8))
        group = np.array([0, 0, 1, 1], np.int32)
        with pytest.raises(GpcaError) as ei:
            e.f2_blocks(group, np.zeros(M, np.int32), 2, 1)
        assert ei.value.status == _lib.GPCA_ERR_BAD_ARG and "2^21" in str(ei.value) and "gpca_f2_blocks" in str(ei.value)
        acc, cnt = e.f2_blocks(group, np.zeros(M - 1, np.int32), 2, 1, rows=(1, M))      # 2^21 rows are served
        assert 0 < cnt[0, 0] <= M - 1


def test_the_timing_record():
    G, group = make(64, 300, 2, seed=1900)
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        load(e, G)
        e.enable_timings(True)
        e.reset_timings()
        e.f2_blocks(group, np.zeros(64, np.int32), 2, 1)
        recs = e.timings()
        assert recs["f2_blocks"]["launches"] == 1 and recs["group_counts"]["launches"] == 1
