"""gpca_sample_counts (sample_counts.hip, gpca_sample_counts.cpp; include/gpca.h section a18) through the C ABI against a numpy model.

The counts and the weighted sums are exact integers, so every comparison is ``array_equal``.  The model (``model``): per sample, the
kept rows with a call other than missing, with call 1 and with call 2, and the uint64 sum of q over the rows with a call.

Shapes: the sample counts around the thread's 16 samples, 32, 64, kSamplePad (256), the wave's chunk of 1 024 samples (kScChunk,
plan_math.h; = kSamplePad2bit) and two chunks, down to one sample, at 33 rows; the row counts 1, 254 .. 257 and 511 and the ones
around the byte counters' flush every 248 rows (kScFlushRows) and its fetch groups of 8 at 257 samples, with a sample that is het on
every row, one that is hom2 on every row and one that is missing on every row; the keep masks of tests/_edges.py; every forced split
count (GPCA_SAMPLE_COUNTS_SPLITS) in {1, 2, 3, 7, rows} at 600 x 257 and 5 x 33 against the default plan; weights of 2^30 over 9 rows
(the sum passes 2^32) and random ones; no, some and only missing calls; one missing call at a time at every sample of the first 64
and the first of the next chunk; both storages and an f32-precision handle; every split of a 70-row call into two bands; and a18's
error list, with an invalid byte below N and pad codes that count nothing."""
import ctypes

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from genomic_pca_amd._lib import GpcaError

from _edges import edge_keeps

pytestmark = pytest.mark.gpu

STORES = {"int8": _lib.STORE_INT8, "2bit": _lib.STORE_2BIT}
SC_CHUNK = 1024       # kScChunk (plan_math.h): the samples of one workgroup
SC_FLUSH = 248        # kScFlushRows
NS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, SC_CHUNK + 1, 2 * SC_CHUNK + 1]
MS = [1, 254, 255, 256, 257, 511, 7, 8, 9, SC_FLUSH - 1, SC_FLUSH, SC_FLUSH + 1, 2 * SC_FLUSH, 2 * SC_FLUSH + 1]
QMAX = 1 << 30


def make(M, N, seed, miss=0.02, fixture=False):
    """M rows x N samples, a fraction `miss` of the calls missing; random weights up to 2^30.  fixture: sample 0 is het on every row,
    sample 1 hom2 on every row, sample 2 missing on every row (where N allows)"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.95, M)[:, None]
    G = (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)
    G[rng.random((M, N)) < miss] = -127
    if fixture:
        for n, v in enumerate((1, 2, -127)):
            if n < N:
                G[:, n] = v
    q = rng.integers(0, QMAX + 1, M).astype(np.uint32)
    q[0] = QMAX
    return G, q


def model(G, q=None, keep=None):
    """(uint32 [N][3] = n_obs, n_het, n_hom2; uint64 [N] or None)"""
    k = np.ones(G.shape[0], bool) if keep is None else np.asarray(keep) != 0
    Gk = G[k]
    obs = Gk != -127
    counts = np.stack([obs.sum(0), (Gk == 1).sum(0), (Gk == 2).sum(0)], 1).astype(np.uint32)
    qs = None if q is None else obs.T.astype(np.uint64) @ np.asarray(q, np.uint64)
    return counts, qs


def load(e, G, keep=None):
    e.upload_genotypes_i8(G)
    M = G.shape[0]
    e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.ones(M, np.uint8) if keep is None else keep)


def check(e, G, q, keep=None, rows=None, what=None):
    """both forms of the call against the model; q: the weights of the kept rows (of the band `rows` of them, where one is given), or
    None for the form without weights alone"""
    if rows is not None:                                      # the model of a band: the keep mask of its kept rows only
        kr = np.flatnonzero(np.ones(G.shape[0], np.uint8) if keep is None else keep)[rows[0]:rows[1]]
        keep = np.zeros(G.shape[0], np.uint8); keep[kr] = 1
    wc, wq = model(G, q, keep)
    if q is not None:
        r = e.sample_counts(q, rows=rows)
        assert r["counts"].dtype == np.uint32 and r["qsum"].dtype == np.uint64 and r["counts"].shape == (G.shape[1], 3)
        assert np.array_equal(r["counts"], wc) and np.array_equal(r["qsum"], wq), what
    r = e.sample_counts(rows=rows)
    assert r["counts"].dtype == np.uint32 and r["counts"].shape == (G.shape[1], 3)
    assert r["qsum"] is None and np.array_equal(r["counts"], wc), what


@pytest.mark.parametrize("store", sorted(STORES))
def test_sample_counts(store):
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        for i, N in enumerate(NS):
            G, q = make(33, N, seed=100 + i)
            load(e, G)
            check(e, G, q, what=N)


@pytest.mark.parametrize("store", sorted(STORES))
def test_row_counts_saturate_the_byte_counters(store):
    N = 257
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        for i, M in enumerate(MS):
            G, q = make(M, N, seed=200 + i, fixture=True)
            load(e, G)
            wc, _ = model(G, q)
            assert tuple(wc[0]) == (M, M, 0) and tuple(wc[1]) == (M, 0, M) and tuple(wc[2]) == (0, 0, 0)
            check(e, G, q, what=M)


@pytest.mark.parametrize("store", sorted(STORES))
def test_keep_masks(store):
    M, N = 257, 257
    G, q = make(M, N, seed=210, fixture=True)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        for name, keep in edge_keeps(M):
            load(e, G, keep)
            check(e, G, q[keep != 0], keep, what=name)


@pytest.mark.parametrize("shape", [(600, 257), (5, 33)])
def test_every_forced_split_gives_the_default_plan_s_bits(shape, monkeypatch):
    M, N = shape
    G, q = make(M, N, seed=300 + M, fixture=True)
    wc, wq = model(G, q)
    for store in sorted(STORES):
        monkeypatch.delenv("GPCA_SAMPLE_COUNTS_SPLITS", raising=False)
        with gpca.GpcaEngine(storage=STORES[store]) as e:
            load(e, G)
            base = e.sample_counts(q)
        assert np.array_equal(base["counts"], wc) and np.array_equal(base["qsum"], wq)
        for s in (1, 2, 3, 7, M, 10 * M, 0):                  # (above the rows and below 1: clamped)
            monkeypatch.setenv("GPCA_SAMPLE_COUNTS_SPLITS", str(s))   # before the engine is created; the library reads it per call
            with gpca.GpcaEngine(storage=STORES[store]) as e:
                load(e, G)
                r = e.sample_counts(q)
                assert np.array_equal(r["counts"], base["counts"]) and np.array_equal(r["qsum"], base["qsum"]), (store, s)
                assert np.array_equal(e.sample_counts()["counts"], base["counts"]), (store, s)
                a, b = e.sample_counts(q[:M // 2], rows=(0, M // 2)), e.sample_counts(q[M // 2:], rows=(M // 2, M))
                assert np.array_equal(a["counts"] + b["counts"], wc) and np.array_equal(a["qsum"] + b["qsum"], wq), (store, s)


@pytest.mark.parametrize("store", sorted(STORES))
def test_the_weighted_sum_carries_into_64_bits(store):
    M, N = 9, 40
    G, _ = make(M, N, seed=400, miss=0.1)
    G[:, 0] = 0                                               # observed on every row: 9 x 2^30 > 2^32
    q = np.full(M, QMAX, np.uint32)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        load(e, G)
        r = e.sample_counts(q)
        assert int(r["qsum"][0]) == 9 * QMAX > 1 << 32
        check(e, G, q)
        check(e, G, np.zeros(M, np.uint32))


@pytest.mark.parametrize("store", sorted(STORES))
def test_missing_rates(store):
    N, M = 130, 33
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        for miss in (0.0, 0.02, 1.0):
            G, q = make(M, N, seed=500, miss=miss)
            assert (miss == 0.0) == (not (G == -127).any()) and (miss == 1.0) == bool((G == -127).all())
            load(e, G)
            check(e, G, q, what=miss)
            if miss == 1.0:
                r = e.sample_counts(q)
                assert not r["counts"].any() and not r["qsum"].any()


@pytest.mark.parametrize("store", sorted(STORES))
def test_one_missing_call_at_every_sample_of_a_wave_and_the_first_of_the_next(store):
    """an otherwise complete matrix: the per-sample weighted work runs on exactly one row of one wave"""
    N, M = SC_CHUNK + 6, 9
    G0, q = make(M, N, seed=600, miss=0.0)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        for n in list(range(65)) + [SC_CHUNK - 1, SC_CHUNK, N - 1]:
            G = G0.copy()
            G[5, n] = -127
            load(e, G)
            wc, wq = model(G, q)
            assert wc[n, 0] == M - 1 and wc[:, 0].sum() == M * N - 1
            r = e.sample_counts(q)
            assert np.array_equal(r["counts"], wc) and np.array_equal(r["qsum"], wq), n


def test_storages_and_precisions_agree():
    G, q = make(2 * SC_FLUSH + 3, 1025, seed=700, fixture=True)
    wc, wq = model(G, q)
    for store, prec in (("int8", _lib.PREC_I8_EXACT), ("2bit", _lib.PREC_I8_EXACT), ("int8", _lib.PREC_F32_MFMA)):
        with gpca.GpcaEngine(precision=prec, storage=STORES[store]) as e:
            load(e, G)
            r = e.sample_counts(q)
            assert np.array_equal(r["counts"], wc) and np.array_equal(r["qsum"], wq), (store, prec)


@pytest.mark.parametrize("store", sorted(STORES))
def test_every_band_split_of_a_70_row_call(store):
    G, q = make(70, 257, seed=800)
    wc, wq = model(G, q)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        load(e, G)
        full = e.sample_counts(q)
        assert np.array_equal(full["counts"], wc) and np.array_equal(full["qsum"], wq)
        for s in range(71):
            a, b = e.sample_counts(q[:s], rows=(0, s)), e.sample_counts(q[s:], rows=(s, 70))
            assert np.array_equal(a["counts"] + b["counts"], wc) and np.array_equal(a["qsum"] + b["qsum"], wq), s
        assert not e.sample_counts(q[:0], rows=(7, 7))["counts"].any()              # an empty band writes zeros


def test_the_sample_mask_is_ignored_and_no_fitted_result_is_touched():
    G, q = make(300, 200, seed=850, miss=0.0)
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        e.upload_genotypes_i8(G)
        e.snp_stats(gpca.QcConfig.none())
        mask = np.zeros(200, np.uint8); mask[::2] = 1
        e.set_sample_mask(mask)
        e.rsvd(4, 4, 1, seed=3)
        sc, ev = e.scores(f64=True).copy(), e.eigenvalues().copy()
        r = e.sample_counts(q)
        wc, wq = model(G, q)
        assert np.array_equal(r["counts"], wc) and np.array_equal(r["qsum"], wq)
        assert np.array_equal(e.scores(f64=True), sc) and np.array_equal(e.eigenvalues(), ev)


def test_pad_codes_of_a_bed_row_count_nothing():
    """.bed rows whose last byte holds codes past N (het, hom, missing): 2-bit residency keeps what the file holds"""
    N, M = 13, 40
    rng = np.random.default_rng(900)
    bed = rng.integers(0, 256, (M, (N + 3) // 4)).astype(np.uint8)                   # every code, the three pad slots of byte 3 included
    lut = np.array([2, -127, 1, 0], np.int8)                                         # the .bed codes as calls
    G = lut[(bed[:, np.arange(N) // 4] >> (2 * (np.arange(N) % 4)).astype(np.uint8)) & 3]
    q = rng.integers(0, QMAX + 1, M).astype(np.uint32)
    wc, wq = model(G, q)
    for store in sorted(STORES):
        with gpca.GpcaEngine(storage=STORES[store]) as e:
            e.upload_bed2bit(bed, N)
            assert np.array_equal(e.download_genotypes_i8(), G)
            e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.ones(M, np.uint8))
            r = e.sample_counts(q)
            assert np.array_equal(r["counts"], wc) and np.array_equal(r["qsum"], wq), store


def test_error_paths():
    N, M = 130, 40
    G, q = make(M, N, seed=1000)
    lib = _lib.load()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        with pytest.raises(GpcaError) as ei:                                             # no genotypes
            e.sample_counts()
        assert ei.value.status == _lib.GPCA_ERR_STATE and "gpca_sample_counts" in str(ei.value)
        e.upload_genotypes_i8(G)
        with pytest.raises(GpcaError) as ei:                                             # no standardisation
            e.sample_counts()
        assert ei.value.status == _lib.GPCA_ERR_STATE and "standardisation" in str(ei.value)
        load(e, G)
        check(e, G, q)
        counts, qsum = np.zeros((N, 3), np.uint32), np.zeros(N, np.uint64)

        def raw(r0, r1, qq, c, s):
            rc = lib.gpca_sample_counts(e._h, r0, r1, None if qq is None else vp(qq), None if c is None else vp(c), None if s is None else vp(s))
            return rc, lib.gpca_last_error(e._h).decode()
        assert raw(0, M, q, counts, qsum)[0] == _lib.GPCA_OK and raw(0, M, None, counts, None)[0] == _lib.GPCA_OK
        big = q.copy(); big[7] = QMAX + 1
        for got, word in ((raw(0, M, q, None, qsum), "counts"), (raw(0, M, q, counts, None), "qsum"), (raw(0, M, None, counts, qsum), "qsum"),
                          (raw(0, M, big, counts, qsum), "q[7]"), (raw(-1, M, q, counts, qsum), "rows"), (raw(3, 2, q, counts, qsum), "rows"),
                          (raw(0, M + 1, q, counts, qsum), "rows")):
            assert got[0] == _lib.GPCA_ERR_BAD_ARG and word in got[1] and "gpca_sample_counts" in got[1], got
        counts[:] = 7
        assert raw(5, 5, None, counts, None)[0] == _lib.GPCA_OK and not counts.any()     # an empty band: written, not added to
        # an invalid byte below N names its row; a band that does not read the row is served
        for bad in (3, -128, -126, 4, 64):
            Gb = G.copy(); Gb[17, N - 1] = bad
            load(e, Gb)
            with pytest.raises(GpcaError) as ei:
                e.sample_counts(q)
            assert ei.value.status == _lib.GPCA_ERR_INVALID_GENOTYPE and "row 17" in str(ei.value), bad
            r = e.sample_counts(q[:17], rows=(0, 17))
            wc, wq = model(Gb[:17], q[:17])
            assert np.array_equal(r["counts"], wc) and np.array_equal(r["qsum"], wq)
        # K = 0: an empty keep mask
        e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.zeros(M, np.uint8))
        with pytest.raises(GpcaError) as ei:
            e.sample_counts()
        assert ei.value.status == _lib.GPCA_ERR_STATE and "no kept row" in str(ei.value)
    # (GPCA_ERR_OOM and a band of 2^31 rows need a matrix no quick test can hold)
    with gpca.GpcaEngine() as e:                                                         # a streamed handle
        e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), M, N, panel_rows=256, ring_slots=2, fused=False)
        e.snp_stats(gpca.QcConfig.none())
        with pytest.raises(GpcaError) as ei:
            e.sample_counts()
        assert ei.value.status == _lib.GPCA_ERR_STATE and "panel" in str(ei.value)
    with gpca.GpcaEngine() as e:                                                         # a hooked (row-sharded) handle
        e.upload_genotypes_i8(G[:20].copy())
        e.set_allreduce_hook(lambda buf: None, 2, 0, 0)
        e.set_standardization(np.ones(20, np.float32), np.ones(20, np.float32), np.ones(20, np.uint8))
        with pytest.raises(GpcaError) as ei:
            e.sample_counts()
        assert ei.value.status == _lib.GPCA_ERR_STATE and "shard" in str(ei.value)


def test_the_timing_record():
    G, q = make(64, 300, seed=1100)
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        load(e, G)
        e.enable_timings(True)
        e.reset_timings()
        e.sample_counts(q)
        recs = e.timings()
        assert "sample_counts" in recs and recs["sample_counts"]["launches"] == 1
