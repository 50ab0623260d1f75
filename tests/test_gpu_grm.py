"""gpca_grm: the genetic relationship matrix of the kept rows (grm.hip, gpca_grm.cpp).

The semantics every layer implements, restated in numpy f64 (``ref_grm``) from the handle's own f32 mu, r = 1 / sigma, b = -mu r:
    Z[i][n] = r_i g + b_i (standardized) or g - mu_i (centred) for an observed call, 0 for a missing one
    GRM[j][k] = (1 / K) sum over the K kept rows of Z[i][j] Z[i][k];  NPAIRS[j][k] = kept rows where j and k are both observed."""
import os
import threading

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from genomic_pca_amd._lib import GpcaError
from _edges import edge_keeps, edge_shapes
from test_gpu_grm_exact import check_device, flush_groups, grm_model

pytestmark = pytest.mark.gpu

STORES = {"int8": _lib.STORE_INT8, "2bit": _lib.STORE_2BIT}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def genotypes(M, N, seed, miss=0.0, dead_sample=None):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.02, 0.5, size=(M, 1))
    G = (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)
    if miss > 0:
        G[rng.random((M, N)) < miss] = -127
    if dead_sample is not None:
        G[:, dead_sample] = -127
    return G


def scale(st):
    """r, b as gpca_set_standardization makes them (f32 1 / sigma, f32 -mu r; 0 on rows that are not kept)"""
    mu, sigma, keep = st["mu"], st["sigma"], st["keep"].astype(bool)
    ok = keep & ~(np.abs(sigma) < np.float32(1e-9))
    r = np.where(ok, np.float32(1.0) / np.where(ok, sigma, np.float32(1)), np.float32(0)).astype(np.float32)
    b = np.where(ok, (-mu * r).astype(np.float32), np.float32(0)).astype(np.float32)
    return r, b


def ref_grm(G, st, scaling):
    keep = st["keep"].astype(bool)
    X = G[keep]
    obs = X != -127
    if scaling == "standardized":
        r, b = scale(st)
        Z = X.astype(np.float64) * r[keep].astype(np.float64)[:, None] + b[keep].astype(np.float64)[:, None]
    else:
        Z = X.astype(np.float64) - st["mu"][keep].astype(np.float64)[:, None]
    Z = np.where(obs, Z, 0.0)
    K = Z.shape[0]
    o = obs.astype(np.float64)
    return (Z.T @ Z) / K, o.T @ o


_MODELS = {}


def model_check(key, G, st, scaling, g, npairs, P, ranks=1):
    """the exact integer model of test_gpu_grm_exact.py next to the f64 bar: equality where every integer stays below 2^53, the per-element
    rounding bar elsewhere.  One model is kept at a time (they are large): the resident and the streamed call of a case share it."""
    hit = _MODELS.get(key)
    if hit is None or not all(np.array_equal(hit[0][k], st[k], equal_nan=True) for k in ("mu", "sigma", "keep")):
        _MODELS.clear()
        hit = _MODELS[key] = ({k: np.array(v) for k, v in st.items()}, grm_model(G, st["mu"], st["sigma"], st["keep"], scaling))
    il = np.tril_indices(G.shape[1])
    return check_device(g[il], None if npairs is None else npairs[il], hit[1], P, key, ranks=ranks)


def keep_some(e, seed, frac=0.9):
    st = e.snp_stats()
    M = e.dims()[0]
    keep = st["keep"].astype(np.uint8) & (np.random.default_rng(seed).random(M) < frac).astype(np.uint8)
    e.set_standardization(st["mu"], st["sigma"], keep)
    return e.get_standardization()


# 1. both scalings against numpy (several flush groups of 4 096 rows)
@pytest.mark.parametrize("store", ["int8", "2bit"])
@pytest.mark.parametrize("N", [200, 1500, 2085])
@pytest.mark.parametrize("miss", [0.0, 0.02])
def test_matches_numpy(store, N, miss):
    M = 9500
    G = genotypes(M, N, seed=N + int(miss * 100), miss=miss, dead_sample=N // 3 if miss else None)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.upload_genotypes_i8(G)
        st = keep_some(e, seed=N)
        for scaling in ("standardized", "centred"):
            g, npairs = e.grm(scaling, npairs=True)
            ref, ref_np = ref_grm(G, st, scaling)
            assert g.shape == (N, N) and np.array_equal(g, g.T)
            assert np.max(np.abs(g - ref)) <= 1e-8 * np.max(np.diag(ref)), scaling
            assert np.array_equal(npairs, ref_np.astype(np.float32))
            model_check(("numpy", N, miss, scaling), G, st, scaling, g, npairs, flush_groups(M))
            if miss:
                assert np.all(npairs[N // 3] == 0) and np.max(np.abs(g[N // 3])) <= 1e-8 * np.max(np.diag(ref))


# 2. int8 and 2-bit storage: the same bits
def test_int8_and_2bit_bit_identical():
    M, N = 6000, 1100
    G = genotypes(M, N, seed=5, miss=0.02)
    out = []
    for store in ("int8", "2bit"):
        with gpca.GpcaEngine(storage=STORES[store]) as e:
            e.upload_genotypes_i8(G)
            keep_some(e, seed=6)
            out.append([e.grm(s, npairs=True) for s in ("standardized", "centred")])
    for (ga, na), (gb, nb) in zip(out[0], out[1]):
        assert np.array_equal(ga, gb) and np.array_equal(na, nb)


# 3. row bands are bit-identical to the same rows of the full call
@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_bands_bit_identical(store):
    M, N, r = 5000, 1500, 777
    G = genotypes(M, N, seed=7, miss=0.02)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.upload_genotypes_i8(G)
        keep_some(e, seed=8)
        for s in ("standardized", "centred"):
            full, fnp = e.grm(s, rows=(0, N), npairs=True)
            a, anp = e.grm(s, rows=(0, r), npairs=True)
            b, bnp = e.grm(s, rows=(r, N), npairs=True)
            assert full.size == N * (N + 1) // 2 and a.size == r * (r + 1) // 2
            assert np.array_equal(np.concatenate([a, b]), full) and np.array_equal(np.concatenate([anp, bnp]), fnp)
            sq = e.grm(s)
            assert np.array_equal(sq[np.tril_indices(N)], full)


# 4. streamed equals resident: bit for bit with panels of a multiple of the flush group, 1e-12 otherwise -- and, while every integer of the
#    call stays below 2^53, bit for bit whatever the panels are (exact integers do not depend on the grouping): model_check asserts it
@pytest.mark.parametrize("store", ["int8", "2bit"])
@pytest.mark.parametrize("panel_rows,exact", [(8192, True), (3072, False)])
def test_streamed_equals_resident(store, panel_rows, exact):
    M, N = 20000, 700
    G = genotypes(M, N, seed=9, miss=0.01)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.upload_genotypes_i8(G)
        st = keep_some(e, seed=10)
        res = [e.grm(s, npairs=True) for s in ("standardized", "centred")]
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), M, N, panel_rows=panel_rows, ring_slots=2, fused=False)
        e.snp_stats()
        e.set_standardization(st["mu"], st["sigma"], st["keep"])
        strm = [e.grm(s, npairs=True) for s in ("standardized", "centred")]
        pr = e.stream_info()["panel_rows"]
    for (g, n), (gs, ns), scaling in zip(res, strm, ("standardized", "centred")):
        assert np.array_equal(n, ns)
        model_check(("streamed", scaling), G, st, scaling, g, n, flush_groups(M))
        model_check(("streamed", scaling), G, st, scaling, gs, ns, flush_groups(M, pr))
        if exact:
            assert np.array_equal(g, gs)
        else:
            assert np.max(np.abs(g - gs)) <= 1e-12 * np.max(np.abs(g))


# 5. two ranks through the allreduce hook on one GPU
def _two_ranks(G, st, scaling, poison=None):
    M = G.shape[0]
    world = 2
    spans = [gpca.shard_rows(M, world, r) for r in range(world)]
    barrier = threading.Barrier(world)
    bufs, res = [None] * world, [None] * world

    def run(rank):
        a, b_ = spans[rank]
        Gr = G[a:b_].copy()
        sg = st["sigma"][a:b_].copy()
        if rank == 1 and poison == "genotype":
            Gr[np.flatnonzero(st["keep"][a:b_])[3], 11] = 3
        if rank == 1 and poison == "sigma":
            sg[np.flatnonzero(st["keep"][a:b_])[3]] = np.nan
        with gpca.GpcaEngine() as e:
            e.upload_genotypes_i8(Gr)

            def hook(buf):
                bufs[rank] = buf.copy(); barrier.wait()
                buf[:] = sum(bufs[r] for r in range(world)); barrier.wait()
            e.set_allreduce_hook(hook, world, rank, a)
            e.set_standardization(st["mu"][a:b_], sg, st["keep"][a:b_])
            try:
                res[rank] = e.grm(scaling, npairs=True)
            except GpcaError as err:
                res[rank] = err
    ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in ts]; [t.join() for t in ts]
    return res


@pytest.mark.parametrize("scaling", ["standardized", "centred"])
def test_two_ranks_hook(scaling):
    M, N = 9000, 500
    G = genotypes(M, N, seed=31, miss=0.02)
    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(G)
        st = keep_some(e, seed=32)
        g1, n1 = e.grm(scaling, npairs=True)
    for g, n in _two_ranks(G, st, scaling):
        assert np.max(np.abs(g - g1)) <= 1e-12 * np.max(np.abs(g1))
        assert np.array_equal(n, n1)
        model_check(("two ranks", scaling), G, st, scaling, g, n, sum(flush_groups(b - a) for a, b in (gpca.shard_rows(M, 2, r) for r in range(2))), ranks=2)
    for poison, code in (("genotype", _lib.GPCA_ERR_INVALID_GENOTYPE), ("sigma", _lib.GPCA_ERR_BAD_ARG)):
        if poison == "sigma" and scaling == "centred":
            continue                                     # (sigma does not enter the centred scaling)
        for r in _two_ranks(G, st, scaling, poison):
            assert isinstance(r, GpcaError) and r.status == code, (poison, r)


# 6. exact PCA from the device GRM
def test_exact_pca_standardized(oracle):
    M, N, k = 6000, 300, 5
    G = genotypes(M, N, seed=41)
    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(G)
        st = e.snp_stats()
        st = e.get_standardization()
        g = e.grm("standardized")
    keep = st["keep"].astype(bool)
    r, b = scale(st)
    E = oracle.exact_pca(G[keep], N, r[keep], b[keep], k)
    K = int(keep.sum())
    w, V = np.linalg.eigh(g * K)
    w = w[::-1][:k]; V = V[:, ::-1][:, :k]
    assert np.max(np.abs(w / (N - 1) - E["eigenvalues"]) / E["eigenvalues"]) <= 1e-6
    sc = oracle.sign_align(V * np.sqrt(w), E["scores"])
    assert np.max(np.abs(sc - E["scores"])) <= 1e-6 * np.max(np.abs(E["scores"]))


def test_exact_pca_centred_chr22(oracle):
    z = np.load(os.path.join(GOLD, "chr22_subset50_120k.npz"))
    rows = z["bed_rows"]; n = int(z["n_samples"])
    lut = np.array([2, -127, 1, 0], np.int8)
    G = np.empty((rows.shape[0], rows.shape[1] * 4), np.int8)
    for s4 in range(4):
        G[:, s4::4] = lut[(rows >> (2 * s4)) & 3]
    G = np.ascontiguousarray(G[:, :n])
    k = 6
    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(G)
        st = e.snp_stats(gpca.QcConfig(0.98, 0.01, 1e-6))
        st = e.get_standardization()
        g = e.grm("centred")
    E = oracle.exact_pca_centred_only(G, n, st["keep"], k)
    w, V = np.linalg.eigh(g)
    w = w[::-1][:k]; V = V[:, ::-1][:, :k]
    assert np.max(np.abs(w - E["evals"]) / E["evals"]) <= 1e-6
    pcs = oracle.sign_align(V * np.sqrt(w), E["pcs"])
    assert np.max(np.abs(pcs - E["pcs"])) <= 1e-6 * np.max(np.abs(E["pcs"]))


# 7. the handle's fitted state is untouched
@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_handle_state_unchanged(store):
    M, N, k = 2600, 700, 6
    G = genotypes(M, N, seed=51)                 # (gpca_rsvd needs a matrix without missing calls)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.upload_genotypes_i8(G)
        e.snp_stats()
        e.rsvd(k, 10, 2, seed=4)
        snap = lambda: [e.scores(), e.scores(f64=True), e.loadings(), e.eigenvalues(), e.transform()] + list(e.get_standardization().values())
        before = snap()
        e.grm("standardized", npairs=True)
        e.grm("centred", rows=(100, 300))
        after = snap()
        for a, b in zip(before, after):
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


# 8. error codes
def test_errors():
    M, N = 700, 300
    G = genotypes(M, N, seed=61)
    lib = _lib.load()
    out = np.empty(N * (N + 1) // 2)
    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(G)
        assert lib.gpca_grm(e._h, 0, 0, N, out.ctypes.data, None) == _lib.GPCA_ERR_STATE      # no standardisation
        e.snp_stats()
        for sc, r0, r1 in ((2, 0, N), (-1, 0, N), (0, -1, N), (0, 5, 5), (0, 10, 3), (0, 0, N + 1)):
            assert lib.gpca_grm(e._h, sc, r0, r1, out.ctypes.data, None) == _lib.GPCA_ERR_BAD_ARG, (sc, r0, r1)
        st = e.get_standardization()
        e.set_standardization(st["mu"], st["sigma"], np.zeros(M, np.uint8))
        assert lib.gpca_grm(e._h, 0, 0, N, out.ctypes.data, None) == _lib.GPCA_ERR_STATE      # K = 0
        assert lib.gpca_grm(e._h, 0, 0, N, None, None) == _lib.GPCA_ERR_BAD_ARG
    Gb = G.copy()
    Gb[17, 40] = 3
    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(Gb)
        e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.ones(M, np.uint8))
        with pytest.raises(GpcaError) as ei:
            e.grm("centred")
        assert ei.value.status == _lib.GPCA_ERR_INVALID_GENOTYPE
        keep = np.ones(M, np.uint8); keep[17] = 0                 # outside the kept rows: fine
        e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), keep)
        e.grm("centred")
    with gpca.GpcaEngine() as e:                                  # a kept row whose mean gpca_grm cannot use: refused, and the row is named
        e.upload_genotypes_i8(G)
        st = e.snp_stats()
        for bad_mu, scalings in ((-0.25, ("standardized",)), (np.inf, ("standardized", "centred"))):
            mu = st["mu"].copy(); mu[123] = bad_mu
            sigma = np.where(st["sigma"] > 0, st["sigma"], np.float32(1)).astype(np.float32)
            for keep123 in (1, 0):
                keep = np.ones(M, np.uint8); keep[123] = keep123
                e.set_standardization(mu, sigma, keep)
                for sc in scalings:
                    rc = lib.gpca_grm(e._h, 0 if sc == "standardized" else 1, 0, N, out.ctypes.data, None)
                    assert rc == (_lib.GPCA_ERR_BAD_ARG if keep123 else _lib.GPCA_OK), (bad_mu, sc, keep123)
                    if keep123:
                        assert "kept row 123 " in lib.gpca_last_error(e._h).decode(), lib.gpca_last_error(e._h)
    Nw = 600_000                                                  # a band that cannot fit in device memory (1.8e11 entries)
    Gw = genotypes(128, Nw, seed=62)
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        e.upload_genotypes_i8(Gw)
        e.snp_stats()
        assert lib.gpca_grm(e._h, 0, 0, Nw, out.ctypes.data, None) == _lib.GPCA_ERR_OOM
        assert "device memory" in lib.gpca_last_error(e._h).decode()
    with gpca.GpcaEngine() as e:                                  # no genotypes
        assert lib.gpca_grm(e._h, 0, 0, 1, out.ctypes.data, None) == _lib.GPCA_ERR_STATE


# 9. tile edges: sample counts at and around the 64 x 64 output tile, kSamplePad (256) and kSamplePad2bit (1 024), down to one sample; row
#    counts at and around the 32-row block and the flush group (4 096), down to one row.  mu / sigma come from the population frequencies,
#    not from the data, so that every row of every shape -- one sample included -- is a usable model row.
def edge_case(M, N, seed, miss=0.02):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.5, size=(M, 1))
    G = (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)
    G[rng.random((M, N)) < miss] = -127
    mu = (2 * p[:, 0]).astype(np.float32)
    sigma = np.sqrt(2 * p[:, 0] * (1 - p[:, 0])).astype(np.float32)
    return G, mu, sigma


@pytest.mark.parametrize("store", ["int8", "2bit"])
@pytest.mark.parametrize("M,N", edge_shapes((65, 1025)))
def test_tile_edges(store, M, N):
    G, mu, sigma = edge_case(M, N, seed=1000 * N + M)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.upload_genotypes_i8(G)
        e.snp_stats(gpca.QcConfig.none())
        for name, keep in edge_keeps(M):
            e.set_standardization(mu, sigma, keep)
            st = e.get_standardization()
            assert np.array_equal(st["keep"].astype(np.uint8), keep), name
            for scaling in ("standardized", "centred"):
                g, npairs = e.grm(scaling, npairs=True)
                ref, ref_np = ref_grm(G, st, scaling)
                assert g.shape == (N, N) and npairs.shape == (N, N) and np.array_equal(g, g.T), (name, scaling)
                assert np.max(np.abs(g - ref)) <= 1e-8 * np.max(np.diag(ref)), (name, scaling)
                assert np.array_equal(npairs, ref_np.astype(np.float32)), (name, scaling)
                model_check(("edges", M, N, name, scaling), G, st, scaling, g, npairs, flush_groups(M))
                tri = e.grm(scaling, rows=(0, N))
                assert tri.shape == (N * (N + 1) // 2,) and np.array_equal(tri, g[np.tril_indices(N)]), (name, scaling)


@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_bands_cut_at_every_tile_edge(store):
    """[0, N) cut at every multiple of the 64-row output tile, and one below and one above it: the bands, concatenated, are the full call"""
    M, N = 2000, 330
    G, mu, sigma = edge_case(M, N, seed=21)
    cuts = sorted({0, N} | {c for t in range(64, N, 64) for c in (t - 1, t, t + 1)})
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.upload_genotypes_i8(G)
        e.snp_stats(gpca.QcConfig.none())
        e.set_standardization(mu, sigma, np.ones(M, np.uint8))
        for s in ("standardized", "centred"):
            full, fnp = e.grm(s, rows=(0, N), npairs=True)
            parts = [e.grm(s, rows=(a, b), npairs=True) for a, b in zip(cuts[:-1], cuts[1:])]
            assert [p[0].size for p in parts] == [b * (b + 1) // 2 - a * (a + 1) // 2 for a, b in zip(cuts[:-1], cuts[1:])]
            assert np.array_equal(np.concatenate([p[0] for p in parts]), full)
            assert np.array_equal(np.concatenate([p[1] for p in parts]), fnp)
