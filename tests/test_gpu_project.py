"""gpca_project: genotypes projected onto a fitted model with missing calls mean-imputed (project.hip, gpca_project.cpp).

The semantics every layer implements, restated in numpy f64 (``ref_project``):
    score[n][c] = sum over model rows i with g[i][n] observed of (g[i][n] - mu_i) / sigma_i * W[i][c]
    n_used[n]   = number of model rows i with g[i][n] observed
A model row is a row whose W row is not all zero; missing = -127 (int8) / code 3 (2-bit)."""
import threading

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from genomic_pca_amd._lib import GpcaError
from _edges import edge_keeps, edge_shapes
from test_gpu_exact_pass import check_against_bars

pytestmark = pytest.mark.gpu

STORES = {"int8": _lib.STORE_INT8, "2bit": _lib.STORE_2BIT}


def genotypes(M, N, seed, miss=0.0):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.5, size=(M, 1))
    G = (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)
    if miss > 0:
        G[rng.random((M, N)) < miss] = -127
    return G


def random_model(M, k, seed, frac_model=0.8):
    rng = np.random.default_rng(seed)
    mu = rng.uniform(0.1, 1.9, M).astype(np.float32)
    sigma = rng.uniform(0.3, 1.0, M).astype(np.float32)
    W = rng.standard_normal((M, k)).astype(np.float32) * np.float32(0.05)
    W[rng.random(M) >= frac_model] = 0.0
    return mu, sigma, W


def ref_project(G, mu, sigma, W):
    model = np.any(W != 0, axis=1)
    obs = (G != -127) & model[:, None]
    Z = np.where(obs, (G.astype(np.float64) - mu.astype(np.float64)[:, None]) / sigma.astype(np.float64)[:, None], 0.0)
    return Z.T @ W.astype(np.float64), obs.sum(axis=0).astype(np.int32)


def close(sc, ref):
    return np.max(np.abs(sc - ref)) <= 1e-4 * np.max(np.abs(ref))


def own_model(e, k):
    st = e.get_standardization()
    M, _ = e.dims()
    W = np.zeros((M, k), np.float32)
    W[e.pca_snp_rows()] = e.loadings()
    return st["mu"], st["sigma"], W


# 1. the handle's own model on clean data: gpca_transform's bits
@pytest.mark.parametrize("store", ["int8", "2bit"])
@pytest.mark.parametrize("N", [200, 1500, 2085])
@pytest.mark.parametrize("k", [1, 20, 40])
def test_bit_identity_with_transform(store, N, k):
    M = 3000
    G = genotypes(M, N, seed=N + k)
    with gpca.GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=STORES[store]) as e:
        e.upload_genotypes_i8(G)
        e.snp_stats()
        e.rsvd(k, 10, 2, seed=3)
        tr = e.transform()
        mu, sigma, W = own_model(e, k)
        sc, used = e.project(mu, sigma, W)
        assert sc.shape == tr.shape
        assert np.array_equal(sc, tr)
        assert np.all(used == np.count_nonzero(np.any(W != 0, axis=1)))


# 2. missing calls against the numpy restatement
@pytest.mark.parametrize("store", ["int8", "2bit"])
@pytest.mark.parametrize("miss", [0.0, 0.01, 0.3])
def test_missing_matches_numpy(store, miss):
    M, N, k = 2500, 777, 20
    G = genotypes(M, N, seed=5, miss=miss)
    mu, sigma, W = random_model(M, k, seed=6)
    model = np.flatnonzero(np.any(W != 0, axis=1))
    G[model[3], :] = -127                  # a model row that is all missing
    G[:, 17] = -127                        # a sample that is all missing
    nonmodel = np.flatnonzero(~np.any(W != 0, axis=1))
    G[nonmodel[:5], ::3] = -127            # missing calls outside the model change nothing
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.upload_genotypes_i8(G)
        sc, used = e.project(mu, sigma, W)
    ref, ref_used = ref_project(G, mu, sigma, W)
    assert close(sc, ref)
    assert np.array_equal(used, ref_used)
    assert np.all(sc[17] == 0.0) and used[17] == 0
    # the same calls with the non-model rows clean: the same bits
    G2 = G.copy(); G2[nonmodel[:5], ::3] = 1
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.upload_genotypes_i8(G2)
        sc2, used2 = e.project(mu, sigma, W)
    assert np.array_equal(sc, sc2) and np.array_equal(used, used2)


def test_invalid_dosage_only_in_model_rows():
    M, N, k = 640, 300, 5
    G = genotypes(M, N, seed=8, miss=0.02)
    mu, sigma, W = random_model(M, k, seed=9)
    nonmodel = np.flatnonzero(~np.any(W != 0, axis=1))
    model = np.flatnonzero(np.any(W != 0, axis=1))
    G[nonmodel[0], 4] = 5                  # outside the model: ignored
    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(G)
        sc, used = e.project(mu, sigma, W)
        ref, ref_used = ref_project(np.where(np.any(W != 0, axis=1)[:, None], G, 0).astype(np.int8), mu, sigma, W)
        assert close(sc, ref) and np.array_equal(used, ref_used)
    G[model[0], 4] = 3                     # inside: refused
    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(G)
        with pytest.raises(GpcaError) as ei:
            e.project(mu, sigma, W)
        assert ei.value.status == _lib.GPCA_ERR_INVALID_GENOTYPE


# 3. flipped rows: 2 - g through mu' = 2 - mu, W' = -W
@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_flipped_rows(store):
    M, N, k = 1800, 640, 12
    G = genotypes(M, N, seed=11, miss=0.05)
    mu, sigma, W = random_model(M, k, seed=12)
    flip = np.random.default_rng(13).random(M) < 0.4
    Gf = G.copy()
    sub = Gf[flip]
    Gf[flip] = np.where(sub == -127, sub, 2 - sub).astype(np.int8)
    muf = np.where(flip, np.float32(2) - mu, mu).astype(np.float32)
    Wf = np.where(flip[:, None], -W, W).astype(np.float32)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.upload_genotypes_i8(G)
        sc, used = e.project(mu, sigma, W)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.upload_genotypes_i8(Gf)
        scf, usedf = e.project(muf, sigma, Wf)
    assert close(scf, sc) and np.array_equal(used, usedf)


# 4. streamed panels give the resident bits
@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_streamed_equals_resident(store):
    M, N, k = 5000, 900, 40
    G = genotypes(M, N, seed=21, miss=0.01)
    G[1023, :] = np.where(np.arange(N) % 7 == 0, -127, G[1023, :])     # missing codes in the last row of the first panel
    G[2047, 5] = -127
    mu, sigma, W = random_model(M, k, seed=22)
    W[1023] = 0.1; W[2047] = -0.05
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.upload_genotypes_i8(G)
        sc, used = e.project(mu, sigma, W)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), M, N, panel_rows=1024, ring_slots=2, fused=False)
        scs, useds = e.project(mu, sigma, W)
    assert np.array_equal(sc, scs) and np.array_equal(used, useds)
    ref, ref_used = ref_project(G, mu, sigma, W)
    assert close(sc, ref) and np.array_equal(used, ref_used)


# 5. two ranks through the allreduce hook on one GPU
def _two_ranks(G, mu, sigma, W, poison_rank=-1):
    M = G.shape[0]
    world = 2
    spans = [gpca.shard_rows(M, world, r) for r in range(world)]
    barrier = threading.Barrier(world)
    bufs, res = [None] * world, [None] * world

    def run(rank):
        a, b_ = spans[rank]
        s = sigma[a:b_].copy()
        if rank == poison_rank:
            s[np.flatnonzero(np.any(W[a:b_] != 0, axis=1))[0]] = np.nan
        with gpca.GpcaEngine() as e:
            e.upload_genotypes_i8(G[a:b_])

            def hook(buf):
                bufs[rank] = buf.copy(); barrier.wait()
                buf[:] = sum(bufs[r] for r in range(world)); barrier.wait()
            e.set_allreduce_hook(hook, world, rank, a)
            try:
                res[rank] = e.project(mu[a:b_], s, W[a:b_])
            except GpcaError as err:
                res[rank] = err
    ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in ts]; [t.join() for t in ts]
    return res


def test_two_ranks_hook():
    M, N, k = 3000, 500, 10
    G = genotypes(M, N, seed=31, miss=0.02)
    mu, sigma, W = random_model(M, k, seed=32)
    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(G)
        sc1, used1 = e.project(mu, sigma, W)
    res = _two_ranks(G, mu, sigma, W)
    for sc, used in res:
        assert np.max(np.abs(sc - sc1)) <= 1e-12 * np.max(np.abs(sc1))
        assert np.array_equal(used, used1)
    res = _two_ranks(G, mu, sigma, W, poison_rank=1)
    for r in res:
        assert isinstance(r, GpcaError) and r.status == _lib.GPCA_ERR_BAD_ARG


# 6. the handle's fitted state is untouched
@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_handle_state_unchanged(store):
    M, N, k = 2600, 700, 6
    G = genotypes(M, N, seed=41)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.upload_genotypes_i8(G)
        e.snp_stats()
        e.rsvd(k, 10, 2, seed=4)
        snap = lambda: [e.scores(), e.scores(f64=True), e.loadings(), e.eigenvalues(), e.transform()] + list(e.get_standardization().values())
        before = snap()
        mu, sigma, W = random_model(M, 9, seed=42)
        e.project(mu, sigma, W)
        after = snap()
        for a, b in zip(before, after):
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


# 7. error codes
def test_errors():
    M, N = 700, 300
    G = genotypes(M, N, seed=51)
    mu, sigma, W = random_model(M, 4, seed=52)
    lib = _lib.load()
    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(G)
        for bad_k in (0, 129):
            Wk = np.zeros((M, max(bad_k, 1)), np.float32)
            sc = np.empty((N, max(bad_k, 1)))
            rc = lib.gpca_project(e._h, mu.ctypes.data, sigma.ctypes.data, Wk.ctypes.data, bad_k, sc.ctypes.data, None)
            assert rc == _lib.GPCA_ERR_BAD_ARG
        s = sigma.copy(); row = int(np.flatnonzero(np.any(W != 0, axis=1))[2]); s[row] = np.nan
        with pytest.raises(GpcaError) as ei:
            e.project(mu, s, W)
        assert ei.value.status == _lib.GPCA_ERR_BAD_ARG and str(row) in ei.value.message
        s = sigma.copy(); s[row] = 0.0
        with pytest.raises(GpcaError) as ei:
            e.project(mu, s, W)
        assert ei.value.status == _lib.GPCA_ERR_BAD_ARG
        s = sigma.copy(); s[np.flatnonzero(~np.any(W != 0, axis=1))[0]] = np.nan   # outside the model: fine
        e.project(mu, s, W)
    with gpca.GpcaEngine() as e:                     # no genotypes
        sc = np.empty((N, 4))
        rc = lib.gpca_project(e._h, mu.ctypes.data, sigma.ctypes.data, W.ctypes.data, 4, sc.ctypes.data, None)
        assert rc == _lib.GPCA_ERR_STATE
    with gpca.GpcaEngine(precision=_lib.PREC_F32_MFMA) as e:
        e.upload_genotypes_i8(G)
        with pytest.raises(GpcaError) as ei:
            e.project(mu, sigma, W)
        assert ei.value.status == _lib.GPCA_ERR_STATE


# 8. PCA.transform(x) on new samples
def test_pca_transform_new_samples():
    M, N, N2, k = 1500, 300, 257, 5
    G = genotypes(M, N, seed=61)
    x = G.T.astype(np.float64)
    model = gpca.PCA()
    model.rfit(x, k, 10, 1, None)
    fitted = model.transform()
    assert np.array_equal(model.transform(x), fitted)
    assert np.array_equal(model.transform(x.astype(np.float32)), fitted)
    G2 = genotypes(M, N2, seed=62, miss=0.03)
    x2 = G2.T.astype(np.float64)
    x2[G2.T == -127] = np.nan
    got = model.transform(x2)
    e = model._eng
    st = e.get_standardization()
    W = np.zeros((M, model.k), np.float32)
    W[e.pca_snp_rows()] = e.loadings()
    ref, _ = ref_project(G2, st["mu"], st["sigma"], W)
    assert got.shape == (N2, model.k) and close(got, ref)
    with pytest.raises(ValueError):
        model.transform(x2[:, :-1])


# 9. tile edges: sample counts at and around the 64-sample block of the sweep, kSamplePad (256) and kSamplePad2bit (1 024), down to one
#    sample; row counts at and around the 32-row block and the 128-row stage, down to one row; 2 % missing calls; three models per shape.
@pytest.mark.parametrize("store", ["int8", "2bit"])
@pytest.mark.parametrize("M,N", edge_shapes((65, 1025)))
def test_tile_edges(store, M, N):
    k = 33                                                          # two 32-column blocks, the second with one live column
    G = genotypes(M, N, seed=1000 * N + M, miss=0.02)
    G[:, N // 2] = -127                                              # a sample with every call missing
    mu, sigma, W0 = random_model(M, k, seed=M + N, frac_model=1.0)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.upload_genotypes_i8(G)
        for name, model in edge_keeps(M):
            W = np.where(model.astype(bool)[:, None], W0, np.float32(0))
            sc, used = e.project(mu, sigma, W)
            ref, ref_used = ref_project(G, mu, sigma, W)
            assert sc.shape == (N, k) and used.shape == (N,), name
            assert np.array_equal(used, ref_used), name
            # the derived bars of one exact pass (tests/test_gpu_exact_pass.py), every sample and column: not close()'s 1e-4
            check_against_bars(sc, G, mu, sigma, W, 4 if store == "int8" else 3, True, f"project {store} M={M} N={N} {name}")
            assert np.all(sc[N // 2] == 0.0) and used[N // 2] == 0, name
