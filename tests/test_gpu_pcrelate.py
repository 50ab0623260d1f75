"""gpca_pcrelate_isaf / gpca_pcrelate: PC-Relate kinship of the kept rows (pcrelate.hip, gpca_pcrelate.cpp), through the C ABI.

The definitions every layer implements, restated in numpy f64 (``design``, ``ref_beta``, ``ref_mu``, ``ref_pairs``).  K kept rows in
PCA-SNP order, N samples, P coordinates V [N][P], a training mask t, tau; g = the call, o = [observed], g' = g o.
  1. x_n = (1, V_n1 / c_1, ..., V_nP / c_P), c_j = the root mean square of column j over the training samples;
     H = (X^T X)^-1 X^T over the training samples, 0 for the others.
  2. mbar_i = the mean of row i's observed training calls;  beta_i = sum_train H_n g'_in + mbar_i sum_train H_n (1 - o_in), summed
     in f64, rounded once to f32; a row with no observed training call has beta = 0.
  3. mu_in = 0.5f * (fmaf chain over j = 0 .. P of beta_ij (float)x_nj, from 0) in f32;  v_in = o_in and mu_in > tau_f and
     mu_in < 1.0f - tau_f.
  4. r = v (g - 2 mu), s = v sqrt(mu (1 - mu));  num_ab = sum_i r_ia r_ib, den_ab = sum_i s_ia s_ib, nsnp_ab = sum_i v_ia v_ib;
     kinship_ab = num_ab / (4 den_ab), NaN when nsnp_ab = 0.  The device sums num and den as f32 fmaf chains over flush groups of
     F = 256 kept rows (kPcrFlushRows, plan_math.h), counted from the first kept row, and adds the groups in f64.

The bars (u = 2^-24, the unit roundoff of f32; e = 2^-53):
  beta: the device rounds once to f32 (u |beta|) a sum of N products accumulated in f64 with fma, whose error is at most
    (N + 8) e sum_n |H_n gt_in| (gt = g' with the mean imputed; the 8 covers the mean, its product and the last fma), and H itself
    comes from a Cholesky solve of a (P + 1) x (P + 1) system with condition number kappa (computed here), whose relative error is
    at most 8 (P + 1) kappa e.  So the bar is u (|beta| + c1 sum_n |H_n gt_in|) with c1 = ((N + 8) + 8 (P + 1) kappa) e / u.
  mu: a chain of P + 1 fmaf (each partial sum rounds once: at most (P + 1) u sum_j |beta_ij x_nj|), an exact halving, and one more u
    for an x that rounds to f32 the other way where c_j differs in its last f64 bit: (P + 2) u sum_j |beta_ij x_nj|.
  num, den: from the device's mu bits the test forms v with the same f32 comparisons and r, s in f64.  The device's r = fl(g - 2 mu)
    carries one rounding (u), so a product of two carries 2 u + u^2; s = fl(sqrt(fl(mu fl(1 - mu)))) carries u (subtraction), u
    (product), halved by the root, plus the root's own rounding of at most 2 u (1 ulp): at most 3 u, so a product of two carries
    6 u + 9 u^2.  The fmaf chain over a flush group of F rows adds at most F u of the group's sum of |terms| (every partial sum
    rounds once), and the f64 sum of the groups adds 2^-53 per group.  With c = 8 both products are covered:
      |d num_ab| <= (F + c) u sum_i |r_ia r_ib|,   |d den_ab| <= (F + c) u sum_i s_ia s_ib,
      |d kinship| <= (d num + 4 |kinship| d den) / (4 (den - d den)).
    (F + c) u = 1.57e-5 < 1 / (2 * 8193) = 6.1e-5 (asserted below): the bar stays under half of one average term at the largest
    shape, and the tests assert that leaving one kept row out of the restatement breaks it for at least one pair.
  nsnp is exact.

What it is for (test_removes_the_ancestry_bias): seed 11, K = 20 000, two populations of 96 founders at F_ST = 0.1, 16 duplicates, 24
children of founder pairs and 24 full sibs of those children; unrelated pairs = every pair of the 256 samples with no pedigree
relation.  With the f64 restatement alone and P = 1 (the first PC of a numpy SVD of the founders' standardised genotypes, every sample
projected) the means are: unrelated within populations -0.0052, across 0.0000 (bound 0.01), parent-offspring 0.2449 and full sibs
0.2452 (bound 0.25 +- 0.02), duplicates 0.4994 (bound 0.5 +- 0.02); with P = 0 the within-population unrelated mean is 0.0496 (bound
> 0.02).  Every bound is met with a factor 2 to spare but one: the within-population mean sits at 0.52 of its bound (a factor 1.9).
It is no sampling noise that a seed could move: allele frequencies fitted on 96 founders per population shift every within-population
estimate by about -1 / (2 * 96) = -0.0052 (the small-sample term GENESIS's scale correction addresses, out of scope here), and the
relatives carry the same shift.  Pooled over all unrelated pairs the mean is -0.0026."""
import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from genomic_pca_amd._lib import GpcaError
from _edges import edge_keeps, edge_shapes

pytestmark = pytest.mark.gpu

STORES = {"int8": _lib.STORE_INT8, "2bit": _lib.STORE_2BIT}
U = 2.0 ** -24
EPS = 2.0 ** -53
F_ROWS = 256          # kPcrFlushRows (plan_math.h; restated in the header comment of pcrelate.hip)
C_PROD = 8.0          # roundings of r, s and their product (module docstring)
assert (F_ROWS + C_PROD) * U < 1.0 / (2 * 8193)
PS = [0, 1, 3, 32]


# ------------------------------------------------------------------------------------------------ inputs
def two_pop_genotypes(M, N, seed, miss=0.0):
    """two populations with different allele frequencies; sample N // 3 has every call missing; row M // 2 has no observed call"""
    rng = np.random.default_rng(seed)
    pop = (np.arange(N) % 2).astype(np.int64)
    p = np.stack([rng.uniform(0.1, 0.9, M), rng.uniform(0.1, 0.9, M)], 1)          # [M][2]
    pn = p[:, pop]
    G = (rng.random((M, N)) < pn).astype(np.int8) + (rng.random((M, N)) < pn).astype(np.int8)
    if miss > 0:
        G[rng.random((M, N)) < miss] = -127
    if N >= 3:
        G[:, N // 3] = -127
    if M >= 3:
        G[M // 2, :] = -127
    return G, pop


def coords(N, P, pop, seed):
    """V [N][P]: the population indicator, then random orthonormal columns"""
    rng = np.random.default_rng(seed + 1000)
    if P == 0:
        return np.zeros((N, 0))
    Q, _ = np.linalg.qr(rng.standard_normal((N, P)))
    V = Q.copy()
    V[:, 0] = pop - pop.mean() + 0.01 * Q[:, 0]
    return np.ascontiguousarray(V)


def train_mask(N, P, seed):
    t = np.ones(N, np.uint8)
    if N >= 2 * P + 8:
        t[np.random.default_rng(seed + 2000).random(N) < 0.1] = 0
    return t


# ------------------------------------------------------------------------------------------------ the f64 restatement
def design(V, train):
    t = np.asarray(train).astype(bool)
    N, P = V.shape
    c = np.sqrt(np.sum(V[t] ** 2, axis=0) / t.sum())
    X = np.hstack([np.ones((N, 1)), V / c])
    A = X[t].T @ X[t]
    H = np.zeros((P + 1, N))
    H[:, t] = np.linalg.solve(A, X[t].T)
    return X, H, np.linalg.cond(A)


def ref_beta(Gk, H, train):
    """(beta [K][P + 1] f64, sum_n |H_n gt_in| [K][P + 1])"""
    t = np.asarray(train).astype(bool)
    o = Gk != -127
    gp = np.where(o, Gk, 0).astype(np.float64)
    cnt = (o & t).sum(1)
    mbar = np.where(cnt > 0, (gp * t).sum(1) / np.maximum(cnt, 1), 0.0)
    m = (~o).astype(np.float64)
    beta = gp @ H.T + mbar[:, None] * (m @ H.T)
    mag = gp @ np.abs(H).T + mbar[:, None] * (m @ np.abs(H).T)
    beta[cnt == 0] = 0.0
    return beta, mag


def ref_mu(beta, X):
    """(mu [K][N] f64 from beta and the f32 design, sum_j |beta_ij x_nj|)"""
    xf = X.astype(np.float32).astype(np.float64)
    b = np.asarray(beta, np.float64)
    return 0.5 * (b @ xf.T), np.abs(b) @ np.abs(xf).T


def valid_f32(Gk, mu32, tau):
    tf = np.float32(tau)
    return (Gk != -127) & (mu32 > tf) & (mu32 < np.float32(1.0) - tf)


def ref_pairs(Gk, mu32, tau, drop=None):
    """num, den, nsnp and the sums of |terms| [N][N] in f64 from the device's mu bits; drop: a kept row left out"""
    v = valid_f32(Gk, mu32, tau)
    if drop is not None:
        v = v.copy(); v[drop] = False
    mu = mu32.astype(np.float64)
    r = np.where(v, Gk.astype(np.float64) - 2.0 * mu, 0.0)
    s = np.where(v, np.sqrt(np.maximum(mu * (1.0 - mu), 0.0)), 0.0)
    vf = v.astype(np.float64)
    ra = np.abs(r)
    return r.T @ r, s.T @ s, np.rint(vf.T @ vf).astype(np.int64), ra.T @ ra


def kin_and_bar(num, den, nsnp, anum):
    with np.errstate(divide="ignore", invalid="ignore"):
        kin = num / (4.0 * den)
        dn, dd = (F_ROWS + C_PROD) * U * anum, (F_ROWS + C_PROD) * U * den
        bar = (dn + 4.0 * np.abs(kin) * dd) / (4.0 * (den - dd))
    kin[nsnp == 0] = np.nan
    return kin, bar


def lower(a):
    return a[np.tril_indices(a.shape[0])]


def load(e, G, keep=None):
    e.upload_genotypes_i8(G)
    M = G.shape[0]
    e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.ones(M, np.uint8) if keep is None else keep)


# ------------------------------------------------------------------------------------------------ 1, 2: beta and mu
@pytest.mark.parametrize("store", ["int8", "2bit"])
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("miss", [0.0, 0.02])
def test_beta_and_mu(store, P, miss):
    M, N = 702, 333
    G, pop = two_pop_genotypes(M, N, seed=10 + P, miss=miss)
    V, t = coords(N, P, pop, seed=P), train_mask(N, P, seed=P)
    G[5, t.astype(bool)] = -127                                   # observed only outside the training set: beta = 0 too
    keep = np.ones(M, np.uint8); keep[::7] = 0
    Gk = G[keep.astype(bool)]
    X, H, kappa = design(V, t)
    rb, mag = ref_beta(Gk, H, t)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        load(e, G, keep)
        mu, beta = e.pcrelate_isaf(V, train=t)
        mu_b, beta_b = e.pcrelate_isaf(V, train=t, rows=(13, 207))
    assert beta.shape == rb.shape and mu.shape == Gk.shape and beta.dtype == np.float32 and mu.dtype == np.float32
    c1 = ((N + 8) + 8 * (P + 1) * kappa) * EPS / U
    bar = U * (np.abs(rb) + c1 * mag)
    err = np.abs(beta.astype(np.float64) - rb)
    print("beta: max err / bar", np.max(err / np.maximum(bar, 1e-300)), "kappa", kappa)
    assert np.all(err <= bar)
    dead = (((Gk != -127) & t.astype(bool)).sum(1) == 0)
    assert dead.sum() >= 2 and np.all(beta[dead] == 0.0) and np.all(mu[dead] == 0.0)
    m64, amag = ref_mu(beta, X)
    errm = np.abs(mu.astype(np.float64) - m64)
    print("mu: max err / bar", np.max(errm / np.maximum((P + 2) * U * amag, 1e-300)))
    assert np.all(errm <= (P + 2) * U * amag)
    assert np.array_equal(mu_b, mu[13:207]) and np.array_equal(beta_b, beta[13:207])


# ------------------------------------------------------------------------------------------------ 3: num, den, kinship at the edges
_SHAPES = edge_shapes([129, 1025])
_REF = {}


def _edge_case(si, ki):
    M, N = _SHAPES[si]
    P = min(PS[si % 4], max(N - 2, 0))
    miss = 0.02 if si % 2 else 0.0
    G, pop = two_pop_genotypes(M, N, seed=100 + si, miss=miss)
    name, keep = edge_keeps(M)[ki]
    if name == "one row" and M >= 3:                              # (row M // 2 is the all-missing one: keep its neighbour)
        keep = np.zeros(M, np.uint8); keep[M // 2 - 1] = 1
    return M, N, P, G, keep, coords(N, P, pop, seed=si), train_mask(N, P, seed=si)


_CASES = [(si, ki) for si in range(len(_SHAPES)) for ki in range(len(edge_keeps(_SHAPES[si][0])))]


@pytest.mark.parametrize("store", ["int8", "2bit"])
@pytest.mark.parametrize("si,ki", _CASES)
def test_pair_sums_at_edge_shapes(store, si, ki):
    M, N, P, G, keep, V, t = _edge_case(si, ki)
    tau = 0.05
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        load(e, G, keep)
        if N < P + 2:                                             # one sample: no regression exists
            with pytest.raises(GpcaError) as ei:
                e.pcrelate(V, train=t, maf_bound=tau)
            assert ei.value.status == _lib.GPCA_ERR_BAD_ARG
            return
        mu, _ = e.pcrelate_isaf(V, train=t)
        kin, ns = e.pcrelate(V, train=t, maf_bound=tau, rows=(0, N), nsnp=True)
    Gk = G[keep.astype(bool)]
    key = (si, ki)
    if key not in _REF:                                           # the restatement, once per case: both storages must give these mu bits
        num, den, nsnp, anum = ref_pairs(Gk, mu, tau)
        v = valid_f32(Gk, mu, tau)
        drop = int(np.argmax(v.sum(1)))
        _REF[key] = (mu.copy(), num, den, nsnp, anum, ref_pairs(Gk, mu, tau, drop=drop))
    mu0, num, den, nsnp, anum, dropped = _REF[key]
    assert np.array_equal(mu, mu0)
    assert np.array_equal(ns, lower(nsnp))
    rk, bar = kin_and_bar(num, den, nsnp, anum)
    rk, bar = lower(rk), lower(bar)
    ok = ~np.isnan(rk)
    assert np.array_equal(np.isnan(kin), ~ok)
    err = np.abs(kin[ok] - rk[ok])
    if ok.any():
        print("kinship: max err / bar", np.max(err / np.maximum(bar[ok], 1e-300)))
    assert np.all(err <= bar[ok])
    if Gk.shape[0] > 1 or ok.any():                               # one kept row left out of the restatement: the bar sees it
        dk, dbar = kin_and_bar(*dropped)
        dk, dbar = lower(dk), lower(dbar)
        both = ok & ~np.isnan(dk)
        broke = np.any(np.isnan(dk) != ~ok) or np.any(np.abs(kin[both] - dk[both]) > dbar[both])
        assert broke


# ------------------------------------------------------------------------------------------------ 4: threshold flips
def test_threshold_flips():
    M, N, P = 600, 200, 3
    G, pop = two_pop_genotypes(M, N, seed=41, miss=0.02)
    V, t = coords(N, P, pop, seed=41), train_mask(N, P, seed=41)
    X, H, kappa = design(V, t)
    rb, mag = ref_beta(G, H, t)
    m64, amag = ref_mu(rb, X)
    xa = np.abs(X.astype(np.float32).astype(np.float64))
    c1 = ((N + 8) + 8 * (P + 1) * kappa) * EPS / U
    # what separates the device's mu from this f64 mu: the item-2 bar, and the beta bar carried through the chain
    margin = (P + 2) * U * amag + 0.5 * (U * (np.abs(rb) + c1 * mag)) @ xa.T
    tau = None
    for k in range(200):                                          # the inputs are chosen: a tau no mu comes near
        cand = 0.05 + 1e-4 * k
        tf = float(np.float32(cand)); omt = float(np.float32(1.0) - np.float32(cand))
        if np.all(np.abs(m64 - tf) > margin) and np.all(np.abs(m64 - omt) > margin):
            tau = cand
            break
    assert tau is not None
    assert np.sum(m64 < tau) > 100 and np.sum(m64 > 1 - tau) > 100      # both thresholds are in use
    with gpca.GpcaEngine() as e:
        load(e, G)
        mu, _ = e.pcrelate_isaf(V, train=t)
        _, ns = e.pcrelate(V, train=t, maf_bound=tau, nsnp=True)
    v_dev = valid_f32(G, mu, tau)
    v_ref = (G != -127) & (m64 > float(np.float32(tau))) & (m64 < float(np.float32(1.0) - np.float32(tau)))
    assert np.array_equal(v_dev, v_ref)
    vf = v_ref.astype(np.float64)
    assert np.array_equal(ns, np.rint(vf.T @ vf).astype(np.int32))


# ------------------------------------------------------------------------------------------------ 5: identities
def _identity_case():
    M, N, P = 1500, 300, 3
    G, pop = two_pop_genotypes(M, N, seed=51, miss=0.02)
    keep = np.ones(M, np.uint8); keep[::5] = 0
    return M, N, P, G, keep, coords(N, P, pop, seed=51), train_mask(N, P, seed=51)


def test_bands_storage_and_precision_bit_identical():
    M, N, P, G, keep, V, t = _identity_case()
    with gpca.GpcaEngine() as e:
        load(e, G, keep)
        full, fn = e.pcrelate(V, train=t, rows=(0, N), nsnp=True)
        for r0 in (0, 1, 127, 128, N - 1):
            r1 = min(N, r0 + 70)
            kb, nb = e.pcrelate(V, train=t, rows=(r0, r1), nsnp=True)
            o0, o1 = r0 * (r0 + 1) // 2, r1 * (r1 + 1) // 2
            assert np.array_equal(kb, full[o0:o1], equal_nan=True) and np.array_equal(nb, fn[o0:o1])
        sq = e.pcrelate(V, train=t)
        assert sq.shape == (N, N) and np.array_equal(sq, sq.T, equal_nan=True) and np.array_equal(lower(sq), full, equal_nan=True)
    with gpca.GpcaEngine(storage=_lib.STORE_2BIT) as e:
        load(e, G, keep)
        k2, n2 = e.pcrelate(V, train=t, rows=(0, N), nsnp=True)
    assert np.array_equal(k2, full, equal_nan=True) and np.array_equal(n2, fn)
    with gpca.GpcaEngine(precision=_lib.PREC_F32_MFMA) as e:
        load(e, G, keep)
        k3, n3 = e.pcrelate(V, train=t, rows=(0, N), nsnp=True)
    assert np.array_equal(k3, full, equal_nan=True) and np.array_equal(n3, fn)
    assert np.isnan(full).sum() == N                              # the all-missing sample: its row and its column


def test_fitted_results_untouched():
    M, N, P, G, keep, V, t = _identity_case()
    G = G.copy(); G[G == -127] = 0
    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(G)
        e.snp_stats()
        e.rsvd(4)
        s0, ev0 = e.scores(f64=True).copy(), e.eigenvalues().copy()
        e.pcrelate(s0[:, :2], maf_bound=0.01)
        e.pcrelate_isaf(s0[:, :2], rows=(0, 10))
        assert np.array_equal(e.scores(f64=True), s0) and np.array_equal(e.eigenvalues(), ev0)


# ------------------------------------------------------------------------------------------------ 6: errors
def _code(fn):
    with pytest.raises(GpcaError) as ei:
        fn()
    return ei.value.status, str(ei.value)


def test_errors():
    M, N = 400, 120
    G, pop = two_pop_genotypes(M, N, seed=61, miss=0.01)
    V = coords(N, 3, pop, seed=61)
    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(G)
        assert _code(lambda: e.pcrelate(V))[0] == _lib.GPCA_ERR_STATE             # no standardisation
        load(e, G)
        assert _code(lambda: e.pcrelate(np.zeros((N, 33))))[0] == _lib.GPCA_ERR_BAD_ARG
        few = np.zeros(N, np.uint8); few[:4] = 1                                  # P + 2 = 5 are needed
        assert _code(lambda: e.pcrelate(V, train=few))[0] == _lib.GPCA_ERR_BAD_ARG
        few[4] = 1
        Vc = V.copy(); Vc[:, 2] = 2.0 * Vc[:, 1]
        assert _code(lambda: e.pcrelate(Vc))[0] == _lib.GPCA_ERR_BAD_ARG          # collinear
        assert _code(lambda: e.pcrelate_isaf(Vc))[0] == _lib.GPCA_ERR_BAD_ARG
        Vn = V.copy(); Vn[7, 1] = np.nan
        assert _code(lambda: e.pcrelate(Vn))[0] == _lib.GPCA_ERR_BAD_ARG
        assert _code(lambda: e.pcrelate(V, maf_bound=0.5))[0] == _lib.GPCA_ERR_BAD_ARG
        assert _code(lambda: e.pcrelate(V, rows=(5, N + 1)))[0] == _lib.GPCA_ERR_BAD_ARG
        assert e.pcrelate(V, maf_bound=0.0).shape == (N, N)
    Gb = G.copy(); Gb[123, 45] = 3
    keep = np.ones(M, np.uint8); keep[17] = 0
    for store in ("int8",):                                                       # (2-bit storage cannot hold a 3)
        with gpca.GpcaEngine(storage=STORES[store]) as e:
            load(e, Gb, keep)
            code, msg = _code(lambda: e.pcrelate(V))
            assert code == _lib.GPCA_ERR_INVALID_GENOTYPE and "row 123" in msg
            code, msg = _code(lambda: e.pcrelate_isaf(V, rows=(0, 4)))
            assert code == _lib.GPCA_ERR_INVALID_GENOTYPE and "row 123" in msg
            keep2 = keep.copy(); keep2[123] = 0                                   # outside the kept rows: fine
            load(e, Gb, keep2)
            e.pcrelate(V)
    with gpca.GpcaEngine() as e:                                                  # a streamed handle
        e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), M, N, panel_rows=256, ring_slots=2, fused=False)
        e.snp_stats(gpca.QcConfig.none())
        code, msg = _code(lambda: e.pcrelate(V))
        assert code == _lib.GPCA_ERR_STATE and "panel" in msg
    with gpca.GpcaEngine() as e:                                                  # a hooked (row-sharded) handle
        e.upload_genotypes_i8(G[:200].copy())
        e.set_allreduce_hook(lambda buf: None, 2, 0, 0)
        e.set_standardization(np.ones(200, np.float32), np.ones(200, np.float32), np.ones(200, np.uint8))
        code, msg = _code(lambda: e.pcrelate(V))
        assert code == _lib.GPCA_ERR_STATE and "shard" in msg


# ------------------------------------------------------------------------------------------------ 7: what it is for
def simulate_cohort(seed=11, K=20000, fst=0.1):
    """(G [K][256] int8, pop, founders mask, pair lists): two populations of 96 founders, 16 duplicates, 24 children, 24 full sibs"""
    rng = np.random.default_rng(seed)
    pa = rng.uniform(0.1, 0.9, K)
    a = (1 - fst) / fst
    p = np.stack([rng.beta(pa * a, (1 - pa) * a) for _ in range(2)], 1)
    nf = 96
    pop = np.repeat([0, 1], nf)
    hap = (rng.random((2, K, 2 * nf)) < p[:, pop][None]).astype(np.int8)           # [2 haplotypes][K][founder]
    cols, pops = [hap[0] + hap[1]], [pop]
    dup_of = np.concatenate([np.arange(8), nf + np.arange(8)])
    cols.append((hap[0] + hap[1])[:, dup_of]); pops.append(pop[dup_of])
    fa = np.concatenate([10 + 2 * np.arange(12), nf + 10 + 2 * np.arange(12)])     # 24 couples, each within one population
    mo = fa + 1

    def child():
        pick_f, pick_m = rng.integers(0, 2, (K, 24)), rng.integers(0, 2, (K, 24))
        return np.where(pick_f == 0, hap[0][:, fa], hap[1][:, fa]) + np.where(pick_m == 0, hap[0][:, mo], hap[1][:, mo])
    cols += [child(), child()]; pops += [pop[fa], pop[fa]]
    G = np.ascontiguousarray(np.concatenate(cols, 1).astype(np.int8))
    pop_all = np.concatenate(pops)
    founders = np.zeros(256, bool); founders[:2 * nf] = True
    c0, s0 = 2 * nf + 16, 2 * nf + 16 + 24
    pairs = {
        "dup": [(2 * nf + i, int(dup_of[i])) for i in range(16)],
        "po": [(c0 + i, int(x[i])) for i in range(24) for x in (fa, mo)] + [(s0 + i, int(x[i])) for i in range(24) for x in (fa, mo)],
        "fs": [(s0 + i, c0 + i) for i in range(24)],
    }
    return G, pop_all, founders, pairs


def cohort_means(kin, pop, founders, pairs):
    """mean kinship of the unrelated pairs (every pair of the 256 samples with no pedigree relation) within and across populations, and
    of each kind of relatives"""
    n = kin.shape[0]
    rel = np.eye(n, dtype=bool)
    for pr in pairs.values():
        for i, j in pr:
            rel[i, j] = rel[j, i] = True
    a, b = np.tril_indices(n, -1)
    un = ~rel[a, b]
    same = pop[a] == pop[b]
    out = {"within": float(np.mean(kin[a[un & same], b[un & same]])), "across": float(np.mean(kin[a[un & ~same], b[un & ~same]]))}
    for k, pr in pairs.items():
        out[k] = float(np.mean([kin[i, j] for i, j in pr]))
    return out


def test_removes_the_ancestry_bias():
    G, pop, founders, pairs = simulate_cohort()
    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(G)
        e.snp_stats()
        e.set_sample_mask(founders.astype(np.uint8))                # the relatives stay out of the fit
        e.rsvd(2)
        pcs = e.transform()[:, :1].astype(np.float64)
        e.set_sample_mask(None)
        k1 = e.pcrelate(pcs, train=founders)
        k0 = e.pcrelate(None, train=founders)
    m1, m0 = cohort_means(k1, pop, founders, pairs), cohort_means(k0, pop, founders, pairs)
    print("P = 1:", m1, " P = 0:", m0)
    assert abs(m1["within"]) <= 0.01 and abs(m1["across"]) <= 0.01
    assert abs(m1["po"] - 0.25) <= 0.02 and abs(m1["fs"] - 0.25) <= 0.02
    assert abs(m1["dup"] - 0.5) <= 0.02
    assert m0["within"] > 0.02
