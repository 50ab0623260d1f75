"""gpca_king: KING-robust kinship of the kept rows (king.hip, gpca_king.cpp).

The semantics every layer implements, restated in numpy (``ref_king``) from the genotypes: per sample and kept row H = [g == 1],
M = [missing], X = g - 1 on homozygous calls; over the K kept rows
    HETHET = sum H_a H_b,  NSNP = K - miss_a - miss_b + sum M_a M_b,  het_ab = het_a - sum H_a M_b,  het_ba = het_b - sum M_a H_b,
    homhom = NSNP - het_ab - het_ba + HETHET,  IBS0 = (homhom - sum X_a X_b) / 2,
    kinship = 0.5 - (4 IBS0 + het_ab + het_ba - 2 HETHET) / (4 min(het_ab, het_ba))   (NaN when the min is 0).
Every intermediate is an exact integer in f64, so the device gives the same bits."""
import threading

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from genomic_pca_amd._lib import GpcaError
from _edges import edge_keeps, edge_shapes

pytestmark = pytest.mark.gpu

STORES = {"int8": _lib.STORE_INT8, "2bit": _lib.STORE_2BIT}


def genotypes(M, N, seed, miss=0.0, special=False):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.02, 0.5, size=(M, 1))
    G = (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)
    if miss > 0:
        G[rng.random((M, N)) < miss] = -127
    if special:
        G[:, N // 3] = np.where(rng.random(M) < 0.5, 0, 2)       # all homozygous: every pair with it has min(het) = 0 -> NaN
        G[:, N // 2] = -127                                       # all missing: NaN too
    return G


def ref_king(G, keep=None):
    """(kinship [N][N], counts [N][N][3] = NSNP, HETHET, IBS0) over the kept rows, exactly as the issue defines them"""
    X = G if keep is None else G[np.asarray(keep).astype(bool)]
    H = (X == 1).astype(np.float64)
    Mi = (X == -127).astype(np.float64)
    Xs = np.where(X == 0, -1.0, np.where(X == 2, 1.0, 0.0))
    K = float(X.shape[0])
    HH, HM, MM, XX = H.T @ H, H.T @ Mi, Mi.T @ Mi, Xs.T @ Xs      # (integers far below 2^53: exact)
    het, miss = H.sum(0), Mi.sum(0)
    nsnp = ((K - miss[:, None]) - miss[None, :]) + MM
    het_ab, het_ba = het[:, None] - HM, het[None, :] - HM.T
    homhom = ((nsnp - het_ab) - het_ba) + HH
    ibs0 = (homhom - XX) / 2
    mn = np.minimum(het_ab, het_ba)
    num = ((4 * ibs0 + het_ab) + het_ba) - 2 * HH
    with np.errstate(divide="ignore", invalid="ignore"):
        kin = 0.5 - num / (4 * mn)
    kin[mn == 0] = np.nan
    return kin, np.stack([nsnp, HH, ibs0], axis=-1).astype(np.int32)


def keep_some(e, seed, frac=0.9):
    st = e.snp_stats()
    M = e.dims()[0]
    keep = st["keep"].astype(np.uint8) & (np.random.default_rng(seed).random(M) < frac).astype(np.uint8)
    e.set_standardization(st["mu"], st["sigma"], keep)
    return e.get_standardization()


def lower(a):
    return a[np.tril_indices(a.shape[0], -1)]


# 1. parity with numpy: counts exact, the kinship bit for bit (several LDS stages, NaN rows from special samples)
@pytest.mark.parametrize("store", ["int8", "2bit"])
@pytest.mark.parametrize("N", [200, 1500, 2085])
@pytest.mark.parametrize("miss", [0.0, 0.02])
def test_matches_numpy(store, N, miss):
    M = 5000
    G = genotypes(M, N, seed=N + int(miss * 100), miss=miss, special=True)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.upload_genotypes_i8(G)
        st = keep_some(e, seed=N)
        kin, cnt = e.king(rows=(0, N), counts=True)
        full = e.king()
    ref, rcnt = ref_king(G, st["keep"])
    assert kin.shape == (N * (N - 1) // 2,) and cnt.shape == (N * (N - 1) // 2, 3)
    assert np.array_equal(cnt, lower(rcnt))
    assert np.array_equal(kin, lower(ref), equal_nan=True)
    assert np.isnan(full[N // 3]).sum() == N - 1 and np.isnan(full[N // 2]).sum() == N - 1
    assert np.array_equal(full, full.T, equal_nan=True) and np.all(np.diag(full) == 0.5)
    assert np.sum(np.isnan(kin)) == np.sum(np.isnan(lower(ref)))


# 1b. the other precision of the handle: the same bits (the kinship reads only the genotypes and the keep mask)
@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_f32_precision_handle(store):
    M, N = 3000, 1100
    G = genotypes(M, N, seed=3, miss=0.02, special=True)
    with gpca.GpcaEngine(precision=_lib.PREC_F32_MFMA, storage=STORES[store]) as e:
        e.upload_genotypes_i8(G)
        st = keep_some(e, seed=4)
        kin, cnt = e.king(counts=True)
    ref, rcnt = ref_king(G, st["keep"])
    assert np.array_equal(lower(kin), lower(ref), equal_nan=True) and np.array_equal(lower(cnt), lower(rcnt))


# 2. row bands are bit-identical to the same rows of the full call (a one-row band, row0 = 0, a band inside a tile)
@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_bands_bit_identical(store):
    M, N = 3000, 1100
    G = genotypes(M, N, seed=7, miss=0.02)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.upload_genotypes_i8(G)
        keep_some(e, seed=8)
        full, fc = e.king(rows=(0, N), counts=True)
        parts = [e.king(rows=b, counts=True) for b in ((0, 1), (1, 2), (2, 300), (300, 301), (301, 777), (777, N))]
        assert parts[0][0].size == 0 and parts[1][0].size == 1 and parts[3][0].size == 300
        assert np.array_equal(np.concatenate([p[0] for p in parts]), full, equal_nan=True)
        assert np.array_equal(np.concatenate([p[1] for p in parts]), fc)


# 3. int8 and 2-bit storage: the same bits
def test_int8_and_2bit_bit_identical():
    M, N = 4000, 1100
    G = genotypes(M, N, seed=5, miss=0.02)
    out = []
    for store in ("int8", "2bit"):
        with gpca.GpcaEngine(storage=STORES[store]) as e:
            e.upload_genotypes_i8(G)
            keep_some(e, seed=6)
            out.append(e.king(counts=True))
    assert np.array_equal(out[0][0], out[1][0], equal_nan=True) and np.array_equal(out[0][1], out[1][1])


# 4. streamed equals resident, bit for bit, for any panel size
@pytest.mark.parametrize("store", ["int8", "2bit"])
@pytest.mark.parametrize("panel_rows", [3072, 8192])
def test_streamed_equals_resident(store, panel_rows):
    M, N = 20000, 700
    G = genotypes(M, N, seed=9, miss=0.01)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.upload_genotypes_i8(G)
        st = keep_some(e, seed=10)
        res = e.king(counts=True)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), M, N, panel_rows=panel_rows, ring_slots=2, fused=False)
        e.snp_stats()
        e.set_standardization(st["mu"], st["sigma"], st["keep"])
        strm = e.king(counts=True)
    assert np.array_equal(res[0], strm[0], equal_nan=True) and np.array_equal(res[1], strm[1])


# 5. two ranks through the allreduce hook on one GPU: the one-rank bits; a poisoned genotype on one rank fails both
def _two_ranks(G, keep, poison=False):
    M = G.shape[0]
    world = 2
    spans = [gpca.shard_rows(M, world, r) for r in range(world)]
    barrier = threading.Barrier(world)
    bufs, res = [None] * world, [None] * world

    def run(rank):
        a, b_ = spans[rank]
        Gr = G[a:b_].copy()
        if rank == 1 and poison:
            Gr[np.flatnonzero(keep[a:b_])[3], 11] = 3
        with gpca.GpcaEngine() as e:
            e.upload_genotypes_i8(Gr)

            def hook(buf):
                bufs[rank] = buf.copy(); barrier.wait()
                buf[:] = sum(bufs[r] for r in range(world)); barrier.wait()
            e.set_allreduce_hook(hook, world, rank, a)
            e.set_standardization(np.ones(b_ - a, np.float32), np.ones(b_ - a, np.float32), keep[a:b_])
            try:
                res[rank] = e.king(counts=True)
            except GpcaError as err:
                res[rank] = err
    ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in ts]; [t.join() for t in ts]
    return res


def test_two_ranks_hook():
    M, N = 9000, 500
    G = genotypes(M, N, seed=31, miss=0.02)
    keep = (np.random.default_rng(32).random(M) < 0.9).astype(np.uint8)
    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(G)
        e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), keep)
        k1, c1 = e.king(counts=True)
    for k, c in _two_ranks(G, keep):
        assert np.array_equal(k, k1, equal_nan=True) and np.array_equal(c, c1)
    for r in _two_ranks(G, keep, poison=True):
        assert isinstance(r, GpcaError) and r.status == _lib.GPCA_ERR_INVALID_GENOTYPE, r


# 6. only kept rows count; the sample mask is ignored
def test_masks():
    M, N = 3000, 400
    G = genotypes(M, N, seed=21, miss=0.02)
    keep = np.zeros(M, np.uint8)
    keep[::3] = 1
    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(G)
        e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), keep)
        k0, c0 = e.king(counts=True)
        mask = np.zeros(N, np.uint8); mask[::2] = 1
        e.set_sample_mask(mask)
        k1, c1 = e.king(counts=True)
    ref, rc = ref_king(G, keep)
    assert np.array_equal(k0, ref, equal_nan=True) and np.array_equal(c0, rc * (1 - np.eye(N, dtype=np.int32))[..., None])
    assert np.array_equal(k0, k1, equal_nan=True) and np.array_equal(c0, c1)
    assert np.all(c0[np.tril_indices(N, -1)][:, 0] <= keep.sum())


# 7. the handle's fitted state is untouched
@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_handle_state_unchanged(store):
    M, N, k = 2600, 700, 6
    G = genotypes(M, N, seed=51)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.upload_genotypes_i8(G)
        e.snp_stats()
        e.rsvd(k, 10, 2, seed=4)
        snap = lambda: [e.scores(), e.scores(f64=True), e.loadings(), e.eigenvalues(), e.transform()] + list(e.get_standardization().values())
        before = snap()
        e.king(counts=True)
        e.king(rows=(100, 300))
        after = snap()
        for a, b in zip(before, after):
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


# 8. error codes
def test_errors():
    M, N = 700, 300
    G = genotypes(M, N, seed=61)
    lib = _lib.load()
    out = np.empty(N * (N - 1) // 2)
    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(G)
        assert lib.gpca_king(e._h, 0, N, out.ctypes.data, None) == _lib.GPCA_ERR_STATE        # no standardisation
        e.snp_stats()
        for r0, r1 in ((-1, N), (5, 5), (10, 3), (0, N + 1)):
            assert lib.gpca_king(e._h, r0, r1, out.ctypes.data, None) == _lib.GPCA_ERR_BAD_ARG, (r0, r1)
        assert lib.gpca_king(e._h, 0, N, None, None) == _lib.GPCA_ERR_BAD_ARG
        st = e.get_standardization()
        e.set_standardization(st["mu"], st["sigma"], np.zeros(M, np.uint8))
        assert lib.gpca_king(e._h, 0, N, out.ctypes.data, None) == _lib.GPCA_ERR_STATE        # K = 0
    Gb = G.copy()
    Gb[17, 40] = 3
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        e.upload_genotypes_i8(Gb)
        e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.ones(M, np.uint8))
        with pytest.raises(GpcaError) as ei:
            e.king()
        assert ei.value.status == _lib.GPCA_ERR_INVALID_GENOTYPE
        keep = np.ones(M, np.uint8); keep[17] = 0                 # outside the kept rows: fine
        e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), keep)
        e.king()
    Nw = 600_000                                                  # a band that cannot fit in device memory (1.8e11 pairs)
    Gw = genotypes(128, Nw, seed=62)
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        e.upload_genotypes_i8(Gw)
        e.snp_stats()
        assert lib.gpca_king(e._h, 0, Nw, out.ctypes.data, None) == _lib.GPCA_ERR_OOM
        assert "device memory" in lib.gpca_last_error(e._h).decode()
    with gpca.GpcaEngine() as e:                                  # no genotypes
        assert lib.gpca_king(e._h, 0, 1, out.ctypes.data, None) == _lib.GPCA_ERR_STATE


# 9. what the feature is for: two Balding-Nichols populations (Fst 0.2) with planted duplicates, parent-offspring and full-sib pairs
def balding_nichols(M=20000, n_pop=150, F=0.2, seed=11):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, M)
    freqs = [rng.beta(p * (1 - F) / F, (1 - p) * (1 - F) / F) for _ in range(2)]
    cols, pop, rel = [], [], {}

    def draw(f):
        return (rng.random(M) < f).astype(np.int8) + (rng.random(M) < f).astype(np.int8)

    def child(x, y):
        hx = np.where(x == 2, 1, np.where(x == 0, 0, rng.integers(0, 2, M)))
        hy = np.where(y == 2, 1, np.where(y == 0, 0, rng.integers(0, 2, M)))
        return (hx + hy).astype(np.int8)
    for k in range(2):
        for _ in range(n_pop):
            cols.append(draw(freqs[k])); pop.append(k)
    for k in range(2):
        s = k * n_pop
        rel[(s, len(cols))] = "dup"; cols.append(cols[s].copy()); pop.append(k)
        P1, P2 = draw(freqs[k]), draw(freqs[k])
        i1 = len(cols); cols += [P1, P2]; pop += [k, k]
        j1 = len(cols); cols += [child(P1, P2), child(P1, P2)]; pop += [k, k]
        for par in (i1, i1 + 1):
            for ch in (j1, j1 + 1):
                rel[(par, ch)] = "po"
        rel[(j1, j1 + 1)] = "fs"
    return np.stack(cols, axis=1), np.array(pop), rel


def test_purpose_relatives_in_structured_cohort():
    G, pop, rel = balding_nichols()
    M, N = G.shape
    mu = G.mean(axis=1).astype(np.float32)
    sd = G.std(axis=1, ddof=1).astype(np.float32)
    keep = (sd > 0).astype(np.uint8)
    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(G)
        e.set_standardization(mu, np.where(keep, sd, np.float32(1)), keep)
        kin = e.king()
        grm = e.grm("standardized")
    assert np.array_equal(kin, ref_king(G, keep)[0], equal_nan=True)
    related = np.zeros((N, N), bool)
    for (i, j), kind in rel.items():
        related[i, j] = related[j, i] = True
        if kind == "dup":
            assert kin[i, j] == 0.5
        else:
            assert 0.177 <= kin[i, j] <= 0.354, (kind, kin[i, j])
    iu = np.triu_indices(N, 1)
    unrel = ~related[iu]
    same = (pop[:, None] == pop[None, :])[iu]
    assert np.max(kin[iu][unrel]) < 0.0442
    # the GRM in kinship units calls unrelated members of one population related on average: why KING is used instead
    assert np.mean(grm[iu][unrel & same] / 2) > 0.0442


# 10. the cutoff workflow's fit: blocks that name only some PCA SNPs make compute_pca narrow the keep mask for the fit and restore it
#     afterwards (which drops the fit); project_all takes every sample's projection before that, and it is the fit of the narrowed
#     keep mask on the masked samples
def test_compute_pca_project_all_with_blocks_leaving_snps_out():
    M, N, k = 4000, 600, 4
    G = genotypes(M, N, seed=71)
    mask = np.ones(N, np.uint8); mask[::7] = 0
    cfg = gpca.EigenSNPCoreAlgorithmConfig(target_num_global_pcs=k, global_pca_sketch_oversampling=6)
    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(G)
        e.snp_stats()
        st = e.get_standardization()
        acc = gpca.MicroarrayGenotypeAccessor(e)
        n_pca = acc.num_pca_snps()
        ids = list(range(0, n_pca, 3)) + list(range(1, n_pca // 2, 3))
        e.set_sample_mask(mask)
        out, _ = gpca.EigenSNPCoreAlgorithm(cfg).compute_pca(acc, [gpca.LdBlockSpecification("b", ids)], project_all=True)
        rows = e.pca_snp_rows()
        after = e.get_standardization()
        assert np.array_equal(after["keep"], st["keep"])                  # the keep mask is restored
    assert out.num_pca_snps_used == len(set(ids)) < n_pca and out.projected_sample_scores.shape == (N, k)
    keep2 = np.zeros_like(st["keep"]); keep2[rows[sorted(set(ids))]] = 1
    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(G)
        e.set_standardization(st["mu"], st["sigma"], keep2)
        e.set_sample_mask(mask)
        e.rsvd(k, 6, cfg.global_pca_num_power_iterations, cfg.random_seed)
        ref = e.transform()
        ev = e.eigenvalues()
    assert np.array_equal(out.projected_sample_scores, ref)
    assert np.array_equal(out.final_principal_component_eigenvalues, ev)
    with gpca.GpcaEngine() as e:                                         # without project_all: nothing extra
        e.upload_genotypes_i8(G)
        e.snp_stats()
        acc = gpca.MicroarrayGenotypeAccessor(e)
        out, _ = gpca.EigenSNPCoreAlgorithm(cfg).compute_pca(acc, [gpca.LdBlockSpecification("b", ids)])
        assert out.projected_sample_scores is None


# 9. tile edges: sample counts at and around the 128 x 128 output tile, kSamplePad (256) and kSamplePad2bit (1 024), down to one sample
#    (an empty triangle); row counts at and around the 32-row block, down to one row; three keep masks per shape.
@pytest.mark.parametrize("store", ["int8", "2bit"])
@pytest.mark.parametrize("M,N", edge_shapes((129, 1025)))
def test_tile_edges(store, M, N):
    G = genotypes(M, N, seed=1000 * N + M, miss=0.02)
    mu, sigma = np.ones(M, np.float32), np.ones(M, np.float32)      # (the kinship reads only the genotypes and the keep mask)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.upload_genotypes_i8(G)
        e.snp_stats(gpca.QcConfig.none())
        for name, keep in edge_keeps(M):
            e.set_standardization(mu, sigma, keep)
            assert np.array_equal(e.get_standardization()["keep"].astype(np.uint8), keep), name
            kin, cnt = e.king(rows=(0, N), counts=True)
            full = e.king()
            ref, rcnt = ref_king(G, keep)
            assert kin.shape == (N * (N - 1) // 2,) and cnt.shape == (N * (N - 1) // 2, 3), name
            assert full.shape == (N, N) and np.all(np.diag(full) == 0.5), name
            assert np.array_equal(cnt, lower(rcnt)), name
            assert np.array_equal(kin, lower(ref), equal_nan=True), name
            assert np.array_equal(lower(full), kin, equal_nan=True) and np.array_equal(full, full.T, equal_nan=True), name


@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_bands_cut_at_every_tile_edge(store):
    """[0, N) cut at every multiple of the 128-row output tile, and one below and one above it: the bands, concatenated, are the full call"""
    M, N = 2000, 530
    G = genotypes(M, N, seed=23, miss=0.02)
    cuts = sorted({0, N} | {c for t in range(128, N, 128) for c in (t - 1, t, t + 1)})
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.upload_genotypes_i8(G)
        keep_some(e, seed=24)
        full, fc = e.king(rows=(0, N), counts=True)
        parts = [e.king(rows=(a, b), counts=True) for a, b in zip(cuts[:-1], cuts[1:])]
        assert [p[0].size for p in parts] == [b * (b - 1) // 2 - a * (a - 1) // 2 for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(np.concatenate([p[0] for p in parts]), full, equal_nan=True)
        assert np.array_equal(np.concatenate([p[1] for p in parts]), fc)
