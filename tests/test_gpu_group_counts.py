"""gpca_group_counts (group_counts.hip, gpca_group_counts.cpp; include/gpca.h section a17) through the C ABI against a numpy model.

The counts are exact integers, so every comparison is ``array_equal``.  The model (``model``): for every kept row, ``np.add.at`` over
(label, call) of the samples with a label >= 0, then n_obs = calls 0 + 1 + 2, n_het = calls 1, n_hom2 = calls 2.

Shapes: the sample counts around the 16-byte operand, the 32-sample ballot block, the 64-sample stage, kSamplePad (256) and
kSamplePad2bit (1 024), down to one sample, at 33 rows; the row counts around the wave's 32 rows and one more than the workgroup's
128 (kGcRows, plan_math.h) at 257 samples; the keep masks of tests/_edges.py; the group counts around the one and the two 32-column
blocks; labels with -1, with an empty group and with everyone in one group; no, some and only missing calls; one missing call at a
time at every sample of the first ballot block and the first of the next; both storages and an f32-precision handle; every split of
a 70-row call into two bands; and a17's error list."""
import ctypes

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from genomic_pca_amd._lib import GpcaError

from _edges import edge_keeps

pytestmark = pytest.mark.gpu

STORES = {"int8": _lib.STORE_INT8, "2bit": _lib.STORE_2BIT}
GC_ROWS = 128         # kGcRows (plan_math.h)
NS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
MS = [1, 31, 32, 33, GC_ROWS + 1]
PS = [1, 2, 31, 32, 33, 63, 64]


def make(M, N, P, seed, miss=0.02, unlabelled=0.1):
    """M rows x N samples of two populations, a fraction `miss` of the calls missing; labels 0 .. P - 1 at random, a fraction
    `unlabelled` of the samples with -1 (or another negative label)"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.95, M)[:, None]
    G = (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)
    G[rng.random((M, N)) < miss] = -127
    group = rng.integers(0, P, N).astype(np.int32)
    group[rng.random(N) < unlabelled] = -1
    if N > 4 and unlabelled > 0:
        group[N // 2] = -7                                    # any negative label is -1
    return G, group


def model(G, group, P, keep=None):
    """uint32 [kept rows][P][3] = n_obs, n_het, n_hom2"""
    Gk = G if keep is None else G[np.asarray(keep) != 0]
    K = Gk.shape[0]
    tab = np.zeros((K, P, 4), np.int64)
    call = np.where(Gk == -127, 3, Gk).astype(np.int64)
    lab = np.flatnonzero(group >= 0)
    rows = np.repeat(np.arange(K), len(lab))
    np.add.at(tab, (rows, np.tile(group[lab], K), call[:, lab].reshape(-1)), 1)
    out = np.stack([tab[..., 0] + tab[..., 1] + tab[..., 2], tab[..., 1], tab[..., 2]], -1)
    return out.astype(np.uint32)


def load(e, G, keep=None):
    e.upload_genotypes_i8(G)
    M = G.shape[0]
    e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.ones(M, np.uint8) if keep is None else keep)


def run(G, group, P, store, keep=None, rows=None, prec=_lib.PREC_I8_EXACT):
    with gpca.GpcaEngine(precision=prec, storage=STORES[store]) as e:
        load(e, G, keep)
        return e.group_counts(group, P, rows=rows)


@pytest.mark.parametrize("store", sorted(STORES))
def test_sample_counts(store):
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        for i, N in enumerate(NS):
            P = (3, 33)[i % 2]
            G, group = make(33, N, P, seed=100 + i)
            load(e, G)
            got = e.group_counts(group, P)
            assert got.dtype == np.uint32 and got.shape == (33, P, 3)
            assert np.array_equal(got, model(G, group, P)), (N, P)


@pytest.mark.parametrize("store", sorted(STORES))
def test_row_counts_and_keep_masks(store):
    N = 257
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        for i, M in enumerate(MS):
            G, group = make(M, N, 5, seed=200 + i)
            load(e, G)
            assert np.array_equal(e.group_counts(group, 5), model(G, group, 5)), M
        G, group = make(GC_ROWS + 1, N, 5, seed=210)
        for name, keep in edge_keeps(GC_ROWS + 1):
            load(e, G, keep)
            got = e.group_counts(group, 5)
            assert got.shape[0] == int(keep.sum()) and np.array_equal(got, model(G, group, 5, keep)), name


@pytest.mark.parametrize("store", sorted(STORES))
def test_group_counts_P(store):
    N = 257
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        for i, P in enumerate(PS):
            G, group = make(33, N, P, seed=300 + i)
            group[:P] = np.arange(P)                          # every group occurs, the last column of the last block included
            load(e, G)
            want = model(G, group, P)
            assert want[:, P - 1, 0].max() > 0
            assert np.array_equal(e.group_counts(group, P), want), P


@pytest.mark.parametrize("store", sorted(STORES))
def test_labels_and_missing_rates(store):
    N, M = 130, 33
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        for miss in (0.0, 0.02, 1.0):
            G, group = make(M, N, 4, seed=400, miss=miss)
            assert (miss == 0.0) == (not (G == -127).any()) and (miss == 1.0) == bool((G == -127).all())
            load(e, G)
            assert np.array_equal(e.group_counts(group, 4), model(G, group, 4)), miss
            empty = np.where(group == 2, 3, group).astype(np.int32)                      # group 2 has no sample
            got = e.group_counts(empty, 4)
            assert np.array_equal(got, model(G, empty, 4)) and not got[:, 2].any()
            one = np.full(N, 1, np.int32)                                                # everyone in one group
            assert np.array_equal(e.group_counts(one, 2), model(G, one, 2))
            nobody = np.full(N, -1, np.int32)
            assert not e.group_counts(nobody, 3).any()
            # n_groups defaults to the largest label + 1
            assert np.array_equal(e.group_counts(group), model(G, group, int(group.max()) + 1))


@pytest.mark.parametrize("store", sorted(STORES))
def test_one_missing_call_at_every_position_of_a_ballot_block(store):
    """an otherwise complete matrix: the missing plane runs in exactly one block of 32 samples of one wave"""
    N, M, P = 70, 33, 3
    G0, group = make(M, N, P, seed=500, miss=0.0, unlabelled=0.0)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        for n in range(33):
            G = G0.copy()
            G[5, n] = -127
            load(e, G)
            want = model(G, group, P)
            assert want[5, :, 0].sum() == N - 1
            assert np.array_equal(e.group_counts(group, P), want), n
        G = G0.copy()
        G[32, N - 1] = -127                                   # the second wave's first row, the last sample
        load(e, G)
        assert np.array_equal(e.group_counts(group, P), model(G, group, P))


def test_storages_and_precisions_agree():
    G, group = make(GC_ROWS + 5, 1025, 40, seed=600)
    want = model(G, group, 40)
    for store in sorted(STORES):
        assert np.array_equal(run(G, group, 40, store), want), store
    assert np.array_equal(run(G, group, 40, "int8", prec=_lib.PREC_F32_MFMA), want)


@pytest.mark.parametrize("store", sorted(STORES))
def test_every_band_split_of_a_70_row_call(store):
    G, group = make(70, 257, 33, seed=700)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        load(e, G)
        full = e.group_counts(group, 33)
        assert np.array_equal(full, model(G, group, 33))
        for s in range(71):
            a, b = e.group_counts(group, 33, rows=(0, s)), e.group_counts(group, 33, rows=(s, 70))
            assert a.shape[0] == s and np.array_equal(np.concatenate([a, b]), full), s


def test_error_paths():
    N, M, P = 130, 40, 3
    G, group = make(M, N, P, seed=800)
    lib = _lib.load()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        e.upload_genotypes_i8(G)
        with pytest.raises(GpcaError) as ei:                                             # no standardisation
            e.group_counts(group, P)
        assert ei.value.status == _lib.GPCA_ERR_STATE and "gpca_group_counts" in str(ei.value)
        load(e, G)
        assert np.array_equal(e.group_counts(group, P), model(G, group, P))
        out = np.zeros((M, P, 3), np.uint32)

        def raw(g, p, r0, r1, o):
            rc = lib.gpca_group_counts(e._h, None if g is None else vp(g), p, r0, r1, None if o is None else vp(o))
            return rc, lib.gpca_last_error(e._h).decode()
        assert raw(group, P, 0, M, out)[0] == _lib.GPCA_OK
        big = group.copy(); big[7] = P
        for got, word in ((raw(None, P, 0, M, out), "group"), (raw(group, P, 0, M, None), "counts"), (raw(group, 0, 0, M, out), "P"),
                          (raw(group, 65, 0, M, out), "P"), (raw(group, -1, 0, M, out), "P"), (raw(big, P, 0, M, out), "group[7]"),
                          (raw(group, P, -1, M, out), "rows"), (raw(group, P, 3, 2, out), "rows"), (raw(group, P, 0, M + 1, out), "rows")):
            assert got[0] == _lib.GPCA_ERR_BAD_ARG and word in got[1] and "gpca_group_counts" in got[1], got
        assert raw(group, P, 5, 5, out)[0] == _lib.GPCA_OK                               # an empty band
        # an invalid byte on a sample with label -1, and on a labelled one
        for lab in (-1, 1):
            Gb = G.copy(); Gb[17, 9] = 3
            gb = group.copy(); gb[9] = lab
            load(e, Gb)
            with pytest.raises(GpcaError) as ei:
                e.group_counts(gb, P)
            assert ei.value.status == _lib.GPCA_ERR_INVALID_GENOTYPE and "row 17" in str(ei.value)
            assert np.array_equal(e.group_counts(gb, P, rows=(0, 17)), model(Gb[:17], gb, P))   # a band that does not read the row
        # K = 0: an empty keep mask
        e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.zeros(M, np.uint8))
        with pytest.raises(GpcaError) as ei:
            e.group_counts(group, P)
        assert ei.value.status == _lib.GPCA_ERR_STATE and "no kept row" in str(ei.value)
    # (GPCA_ERR_OOM needs a band whose counts exceed the free memory of the card: no shape a quick test can hold reaches it)
    with gpca.GpcaEngine() as e:                                                         # a streamed handle
        e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), M, N, panel_rows=256, ring_slots=2, fused=False)
        e.snp_stats(gpca.QcConfig.none())
        with pytest.raises(GpcaError) as ei:
            e.group_counts(group, P)
        assert ei.value.status == _lib.GPCA_ERR_STATE and "panel" in str(ei.value)
    with gpca.GpcaEngine() as e:                                                         # a hooked (row-sharded) handle
        e.upload_genotypes_i8(G[:20].copy())
        e.set_allreduce_hook(lambda buf: None, 2, 0, 0)
        e.set_standardization(np.ones(20, np.float32), np.ones(20, np.float32), np.ones(20, np.uint8))
        with pytest.raises(GpcaError) as ei:
            e.group_counts(group, P)
        assert ei.value.status == _lib.GPCA_ERR_STATE and "shard" in str(ei.value)


def test_the_timing_record():
    G, group = make(64, 300, 2, seed=900)
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        load(e, G)
        e.enable_timings(True)
        e.reset_timings()
        e.group_counts(group, 2)
        recs = e.timings()
        assert "group_counts" in recs and recs["group_counts"]["launches"] == 1
