"""gpca_assoc_linear: the linear association scan of the kept rows (assoc.hip, gpca_assoc.cpp), through the C ABI.

The definitions every layer implements, restated in numpy f64 (``design``, ``restate``, ``finish``).  K kept rows in PCA-SNP order, N
samples, T traits Y, Pc covariates C, an include mask; g = the call, S = the included samples, n = |S|.
  1. Q = an orthonormal basis of the columns of C centred over S (R of Q R with a positive diagonal, which is what the engine's
     Cholesky gives), Y~ = Y centred over S minus Q Q^T Y, B = [Y~ | Q], 0 outside S; yy_t = |Y~_t|^2; df = n - Pc - 2.
  2. o = [observed and in S], g' = g o; n_obs = sum o, s1 = sum g', s2 = sum g'^2; d_ij = sum_n g'_in B_nj, e_ij = sum_n [missing and in
     S] B_nj.  The device multiplies the f32 roundings of B by the calls as f32 (exact products) and sums them in f32 over flush groups
     of F = 256 samples (kAscFlush, plan_math.h) counted from sample 0; the groups are added in f64.
  3. mbar = s1 / n_obs, xb = d + mbar e, xx = s2 - s1 mbar, sxx = xx - sum_{j >= T} xb_j^2, beta = xb_t / sxx, rss = yy_t - xb_t beta,
     se = sqrt(rss / df / sxx), t = beta / se, a1_freq = mbar / 2; NaN when n_obs = 0, xx <= 0, sxx max_vif < xx or rss <= 0.

The bars (u = 2^-24, e = 2^-53, F = 256).  S_ij = sum_n |g'_in B_nj| + mbar sum_miss |B_nj|.
  xb: B rounds once to f32 (u |B|; the products with 0, 1, 2 are then exact).  Within a flush group of at most F terms every partial sum
    rounds once, F u (1 + F u) of the group's sum of |terms|, and a v_mfma_f32_32x32x2_f32 that rounds the sum of its two products before
    it adds them to the accumulator costs one more u of that sum.  First order 1 + F + 1, second order below (F + 2)^2 u = 0.004: with
    c = 3,  |d xb_ij| <= (F + c) u S_ij  from the f32 side.  The f64 side, counted: N / F + 1 additions of groups, the division, the
    product with mbar and the last addition, (N / F + 4) e S_ij; and the host's B against this module's B: the engine's Q comes from
    a Cholesky of the centred unit-norm columns, whose departure from the Householder Q is at most 8 (Pc + 2) kappa^2 e per unit-norm
    column (kappa = the condition number of those columns, computed here), so column j moves xb by at most that times |B_j|_2 times
    sum_n |g~_in| (g~ = g' with the mean imputed).  (F + c) u N = 0.0158 < 1 / 2 at N = 1 025 (asserted): the bar stays under half an
    average term, and every shape asserts that leaving one included sample out of the restatement breaks it somewhere.
  n_obs is exact; a1_freq and xx are the f64 formulas of integers, bit for bit.
  sxx, beta, se, t from the device's own xb in f64 with the order of step 3: the device and numpy may differ by one rounding per
    operation; sxx = xx - q loses at most a factor xx / sxx <= max_vif to cancellation and q is a sum of Pc products, so
    4 (Pc + 2) max_vif e relative covers all four.
  End to end against numpy.linalg.lstsq on the mean-imputed matrix, first order through step 3 with dx = the xb bar:
    d sxx = sum_{j >= T} 2 |xb_j| dx_j;  d beta = (dx_t + |beta| d sxx) / sxx;  d rss = |beta| dx_t + |xb_t| d beta;
    d se = se (d rss / rss + d sxx / sxx) / 2;  d t = |t| (d beta / |beta| + d se / se); each doubled for the second order, plus
    lstsq's own error 64 kappa_X^2 e of the value (kappa_X = the condition number of the row's design, from its singular values).
Every case prints the largest fraction of the xb bar it observes ("xb: max err / bar").

What it is for (test_pc_covariate_removes_inflation): seed 7, N = 600 (two populations of 300 at F_ST = 0.1, Balding-Nichols), K = 3 000
SNPs, y = 1.0 [population 1] + 0.5 g_causal + N(0, 1), causal SNP = row 1 500; PC 1 = the first left singular vector of the standardised
genotypes (numpy SVD).  With the f64 restatement alone, lambda = median t^2 over the other SNPs / 0.4549 (the chi^2_1 median):
  Pc = 1: lambda = 0.9966 (bound |lambda - 1| <= 0.1; measured 0.0034), and the causal SNP is the top hit: t^2 = 38.13 against the
  largest null 16.46 (bound: ratio > 1, measured 2.32, a factor 2.3 to spare);  Pc = 0: lambda = 7.93 (bound >= 3: a factor 2.6)."""
import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from genomic_pca_amd._lib import GpcaError
from _edges import edge_keeps

pytestmark = pytest.mark.gpu

STORES = {"int8": _lib.STORE_INT8, "2bit": _lib.STORE_2BIT}
U = 2.0 ** -24
EPS = 2.0 ** -53
F_ASC = 256           # kAscFlush (plan_math.h; restated in the header comment of assoc.hip)
C_ASC = 3.0           # module docstring
VIF = 50.0
assert (F_ASC + C_ASC) * U * 1025 < 0.5
NS = [4, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
KS = [1, 127, 128, 129, 4097]
TPS = [(1, 0), (1, 31), (32, 0), (16, 16), (1, 32), (33, 31), (64, 0)]


# ------------------------------------------------------------------------------------------------ inputs
def make_inputs(M, N, T, Pc, seed, miss):
    """two populations; sample N // 3 has every call missing; row M // 2 has no observed call; with miss = 0 no other call of an included
    sample is missing (the ballot stays quiet outside that sample's group), and in every other such case (seed a multiple of 4, N large
    enough to exclude anyone) sample N // 3 is an excluded one, so that no row but M // 2 holds a missing call of an included sample and
    the ballot stays quiet across whole rows and flush groups; about one sample in ten is excluded when N allows, and the
    excluded samples hold missing calls and extreme trait and covariate values; from 64 samples and 5 rows on, row 1 is collinear with
    covariate 0 (the VIF rule) and row 2 is monomorphic among the included samples."""
    rng = np.random.default_rng(seed)
    pop = np.arange(N) % 2
    p = np.stack([rng.uniform(0.1, 0.9, M), rng.uniform(0.1, 0.9, M)], 1)[:, pop]
    G = (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)
    inc = np.ones(N, np.uint8)
    if N >= 2 * (Pc + 3) + 8:
        inc[rng.random(N) < 0.1] = 0
        inc[N // 3] = 0 if miss == 0 and seed % 4 == 0 else 1
    if miss > 0:
        G[rng.random((M, N)) < miss] = -127
    G[:, inc == 0] = -127
    if N >= 8:
        G[:, N // 3] = -127
    special = N >= 64 and M >= 5
    if M >= 3:
        G[M // 2, :] = -127
    Y = rng.standard_normal((N, T)) + 0.5 * pop[:, None]
    C = rng.standard_normal((N, Pc))
    if special:
        G[2, inc == 1] = 2
        if Pc:
            o = (G[1] != -127) & (inc == 1)
            C[:, 0] = np.where(G[1] == -127, G[1][o].mean(), G[1]) + 1e-7 * C[:, 0]
    Y[inc == 0] = 1e30
    C[inc == 0] = -1e30
    return G, Y, C, inc, special


# ------------------------------------------------------------------------------------------------ the f64 restatement
def design(Y, C, inc):
    s = np.asarray(inc).astype(bool)
    N, T = Y.shape
    Pc = C.shape[1]
    Cc = C[s] - C[s].mean(0)
    Cc = Cc / np.sqrt((Cc ** 2).sum(0))
    kappa = 1.0
    Q = np.zeros((s.sum(), 0))
    if Pc:
        Q, R = np.linalg.qr(Cc)
        Q = Q * np.sign(np.diag(R))
        sv = np.linalg.svd(Cc, compute_uv=False)
        kappa = sv[0] / sv[-1]
    Yc = Y[s] - Y[s].mean(0)
    Yt = Yc - Q @ (Q.T @ Yc)
    Yt = Yt - Q @ (Q.T @ Yt)
    B = np.zeros((N, T + Pc))
    B[s] = np.hstack([Yt, Q])
    return B, (Yt ** 2).sum(0), int(s.sum()) - Pc - 2, kappa


def restate(Gk, B, inc, kappa, Pc, drop=None):
    s = np.asarray(inc).astype(bool).copy()
    N = Gk.shape[1]
    o = (Gk != -127) & s
    gp = np.where(o, Gk, 0).astype(np.float64)
    ms = ((Gk == -127) & s).astype(np.float64)
    nobs, s1, s2 = o.sum(1), gp.sum(1), (gp * gp).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        mbar = s1 / nobs
    gd, md = gp, ms
    if drop is not None:
        gd, md = gp.copy(), ms.copy(); gd[:, drop] = 0.0; md[:, drop] = 0.0
    mb = np.where(nobs > 0, mbar, 0.0)[:, None]
    with np.errstate(invalid="ignore"):
        xb = gd @ B + mbar[:, None] * (md @ B)
    S = gd @ np.abs(B) + mb * (md @ np.abs(B))
    gt = (gp + mb * ms).sum(1)
    bar = ((F_ASC + C_ASC) * U + (N / F_ASC + 4) * EPS) * S + 8 * (Pc + 2) * kappa ** 2 * EPS * gt[:, None] * np.sqrt((B ** 2).sum(0))[None, :]
    return dict(nobs=nobs, s1=s1, s2=s2, mbar=mbar, xb=xb, bar=bar, gimp=gp + mb * ms)


def finish(xb, nobs, s1, s2, yy, df, T, vif=VIF):
    with np.errstate(all="ignore"):
        mbar = s1 / nobs
        xx = s2 - s1 * mbar
        q = np.zeros(len(xx))
        for j in range(T, xb.shape[1]):
            q = q + xb[:, j] * xb[:, j]
        sxx = xx - q
        beta = xb[:, :T] / sxx[:, None]
        rss = yy[None, :] - xb[:, :T] * beta
        se = np.sqrt(rss / df / sxx[:, None])
        t = beta / se
        dead = ((nobs == 0) | ~(xx > 0) | (sxx * vif < xx))[:, None] | ~(rss > 0)
    beta, se, t = (np.where(dead, np.nan, a) for a in (beta, se, t))
    return dict(a1_freq=mbar / 2, xx=xx, sxx=sxx, beta=beta, se=se, t=t, rss=rss)


def load(e, G, keep=None):
    e.upload_genotypes_i8(G)
    M = G.shape[0]
    e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.ones(M, np.uint8) if keep is None else keep)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def rel_close(got, ref, tol):
    ok = ~np.isnan(ref)
    return same(np.isnan(got), np.isnan(ref)) and np.all(np.abs(got[ok] - ref[ok]) <= tol * np.abs(ref[ok]))


# ------------------------------------------------------------------------------------------------ the edge shapes
def _cases():
    out = []
    i = 0
    for N in NS:
        out.append((4097, N, 2, i)); i += 1
    for M in KS[:-1]:
        for N in (257, 1025):
            for ki in range(len(edge_keeps(M))):
                out.append((M, N, ki, i)); i += 1
    return out


_CASES = _cases()
_REF = {}


def _case(M, N, ki, i):
    T, Pc = TPS[i % len(TPS)]
    Pc = min(Pc, N - 3)                                # df = n - Pc - 2 >= 1 (a small N includes everyone)
    G, Y, C, inc, special = make_inputs(M, N, T, Pc, seed=300 + i, miss=0.03 if i % 2 else 0.0)
    name, keep = edge_keeps(M)[ki]
    if name == "one row" and M >= 3:                   # (row M // 2 is the all-missing one: keep its neighbour)
        keep = np.zeros(M, np.uint8); keep[M // 2 - 1] = 1
    return G, Y, C, inc, keep, T, Pc, special


@pytest.mark.parametrize("store", ["int8", "2bit"])
@pytest.mark.parametrize("M,N,ki,i", _CASES)
def test_scan_at_edge_shapes(store, M, N, ki, i):
    G, Y, C, inc, keep, T, Pc, special = _case(M, N, ki, i)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        load(e, G, keep)
        r = e.assoc_linear(Y, C, include=inc, max_vif=VIF, xb=True)
    Gk = G[keep.astype(bool)]
    K = Gk.shape[0]
    if (i, ki) not in _REF:
        B, yy, df, kappa = design(Y, C, inc)
        ref = restate(Gk, B, inc, kappa, Pc)
        s = inc.astype(bool)
        drop = int(np.flatnonzero(s)[np.argmax(((Gk[:, s] != -127) & (Gk[:, s] != 0)).sum(0))])
        _REF[(i, ki)] = (B, yy, df, kappa, ref, restate(Gk, B, inc, kappa, Pc, drop=drop))
    B, yy, df, kappa, ref, dropped = _REF[(i, ki)]
    assert r["xb"].shape == (K, T + Pc) and r["beta"].shape == (K, T)
    # exact outputs
    assert np.array_equal(r["n_obs"], ref["nobs"].astype(np.float64))
    fin0 = finish(ref["xb"], ref["nobs"], ref["s1"], ref["s2"], yy, df, T)
    assert same(r["a1_freq"], fin0["a1_freq"]) and same(r["xx"], fin0["xx"])
    # xb against the bar
    live = ref["nobs"] > 0
    assert np.all(np.isnan(r["xb"][~live])) and np.all(np.isnan(r["beta"][~live]))
    err = np.abs(r["xb"][live] - ref["xb"][live])
    bar = ref["bar"][live]
    if live.any():
        print("xb: max err / bar", np.max(err / np.maximum(bar, 1e-300)), "kappa", kappa)
    assert np.all(err <= bar)
    if live.any():
        assert np.any(np.abs(r["xb"][live] - dropped["xb"][live]) > dropped["bar"][live])
    # the statistics from the device's own xb
    fin = finish(r["xb"], ref["nobs"], ref["s1"], ref["s2"], yy, df, T)
    tol = 4 * (Pc + 2) * VIF * EPS
    with np.errstate(invalid="ignore"):
        capped = ~(fin["sxx"] * VIF < fin["xx"])           # (where the VIF rule fires the cancellation in sxx has no cap)
    assert rel_close(r["sxx"][capped], fin["sxx"][capped], tol)
    for k in ("beta", "se", "t"):
        assert rel_close(r[k], fin[k], tol), k
    if special and Pc and keep[1]:
        assert np.all(np.isnan(r["beta"][int(keep[:1].sum())]))                 # collinear with covariate 0: the VIF rule
    if special and keep[2]:
        j = int(keep[:2].sum())
        assert r["xx"][j] == 0.0 and np.all(np.isnan(r["t"][j]))                # monomorphic among the included samples
    # end to end: lstsq on the mean-imputed matrix, a spread of rows
    s = inc.astype(bool)
    pick = np.unique(np.linspace(0, K - 1, 24).astype(int))
    Cs = C[s]
    checked = 0
    for k in pick:
        if not np.isfinite(r["beta"][k]).all():
            continue
        X = np.hstack([np.ones((s.sum(), 1)), Cs, ref["gimp"][k, s][:, None]])
        sol, _, _, sv = np.linalg.lstsq(X, Y[s], rcond=None)
        res = Y[s] - X @ sol
        Xn = X / np.sqrt((X ** 2).sum(0))
        svn = np.linalg.svd(Xn, compute_uv=False)
        own = 64 * (svn[0] / svn[-1]) ** 2 * EPS
        b_ref = sol[-1]
        xtx_inv = np.linalg.inv(Xn.T @ Xn)[-1, -1] / (X[:, -1] ** 2).sum()
        se_ref = np.sqrt((res ** 2).sum(0) / df * xtx_inv)
        dx = ref["bar"][k]
        xbk, sxx, beta, se, t = r["xb"][k], r["sxx"][k], r["beta"][k], r["se"][k], r["t"][k]
        rss = yy - xbk[:T] * beta
        dsxx = 2 * np.sum(2 * np.abs(xbk[T:]) * dx[T:])
        dbeta = 2 * (dx[:T] + np.abs(beta) * dsxx) / sxx
        drss = 2 * (np.abs(beta) * dx[:T] + np.abs(xbk[:T]) * dbeta)
        dse = se * (drss / rss + dsxx / sxx)
        dt = 2 * np.abs(t) * (dbeta / np.maximum(np.abs(beta), 1e-300) + dse / se)
        assert np.all(np.abs(beta - b_ref) <= dbeta + own * np.abs(b_ref)), (k, beta, b_ref, dbeta)
        assert np.all(np.abs(se - se_ref) <= dse + own * se_ref), (k, se, se_ref, dse)
        assert np.all(np.abs(t - b_ref / se_ref) <= dt + 2 * own * np.abs(t)), (k,)
        checked += 1
    assert checked or not np.isfinite(r["beta"]).any()


def test_N1_is_refused():
    G = np.ones((5, 1), np.int8)
    with gpca.GpcaEngine() as e:
        load(e, G)
        with pytest.raises(GpcaError) as ei:
            e.assoc_linear(np.ones((1, 1)))
        assert ei.value.status == _lib.GPCA_ERR_BAD_ARG and "df" in str(ei.value)


# ------------------------------------------------------------------------------------------------ identities
def test_bands_storages_precision_and_excluded_samples():
    M, N, T, Pc = 1000, 333, 5, 7
    G, Y, C, inc, _ = make_inputs(M, N, T, Pc, seed=5, miss=0.03)
    keep = np.ones(M, np.uint8); keep[::9] = 0
    K = int(keep.sum())
    out = {}
    for name, kw in (("int8", dict(storage=_lib.STORE_INT8)), ("2bit", dict(storage=_lib.STORE_2BIT)),
                     ("f32", dict(storage=_lib.STORE_INT8, precision=_lib.PREC_F32_MFMA))):
        with gpca.GpcaEngine(**kw) as e:
            load(e, G, keep)
            out[name] = e.assoc_linear(Y, C, include=inc, xb=True)
            if name == "int8":
                bands = [e.assoc_linear(Y, C, include=inc, xb=True, rows=b) for b in ((0, 1), (1, 130), (130, 131), (131, 640), (640, K), (K, K))]
                G2, Y2, C2 = G.copy(), Y.copy(), C.copy()
                x = inc == 0
                assert x.sum() >= 5
                G2[:, x] = np.random.default_rng(1).integers(0, 3, (M, int(x.sum())))
                Y2[x] = -7.0; C2[x] = 3.0
                load(e, G2, keep)
                out["changed"] = e.assoc_linear(Y2, C2, include=inc, xb=True)
    ref = out["int8"]
    assert np.isfinite(ref["t"]).sum() > K * T // 2
    for k in ref:
        assert same(np.concatenate([b[k] for b in bands]), ref[k]), k
        for other in ("2bit", "f32", "changed"):
            assert same(out[other][k], ref[k]), (other, k)


# ------------------------------------------------------------------------------------------------ errors
def test_errors():
    M, N = 40, 50
    rng = np.random.default_rng(3)
    G = rng.integers(0, 3, (M, N)).astype(np.int8)
    Y, C = rng.standard_normal((N, 2)), rng.standard_normal((N, 3))
    lib = _lib.load()

    def status(e, *a, **k):
        with pytest.raises(GpcaError) as ei:
            e.assoc_linear(*a, **k)
        return ei.value.status

    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(G)
        assert status(e, Y, C) == _lib.GPCA_ERR_STATE                                    # no standardisation
        load(e, G, np.zeros(M, np.uint8))
        assert status(e, Y, C) == _lib.GPCA_ERR_STATE                                    # K = 0
        load(e, G)
        BA = _lib.GPCA_ERR_BAD_ARG
        assert status(e, np.zeros((N, 0)), C) == BA                                      # T = 0
        assert status(e, rng.standard_normal((N, 40)), rng.standard_normal((N, 25))) == BA   # T + Pc > 64
        for rows in ((-1, 3), (5, 4), (0, M + 1)):
            assert status(e, Y, C, rows=rows) == BA
        vp = lambda a: a.ctypes.data
        assert lib.gpca_assoc_linear(e._h, vp(Y), 2, vp(C), 3, None, 50.0, 0, M, None, None, None) == BA      # all outputs NULL
        Yn = Y.copy(); Yn[7, 1] = np.nan
        assert status(e, Yn, C) == BA
        inc = np.ones(N, np.uint8); inc[7] = 0
        assert np.isfinite(e.assoc_linear(Yn, C, include=inc)["t"]).all()                # ... but not on an excluded sample
        Cn = C.copy(); Cn[3, 0] = np.inf
        assert status(e, Y, Cn) == BA
        few = np.zeros(N, np.uint8); few[:5] = 1
        assert status(e, Y, C, include=few) == BA                                        # df = 5 - 3 - 2 < 1
        Cc = C.copy(); Cc[:, 1] = 4.0
        assert status(e, Y, Cc) == BA                                                    # a constant column
        Cl = C.copy(); Cl[:, 2] = Cl[:, 0] - 2 * Cl[:, 1]
        assert status(e, Y, Cl) == BA                                                    # collinear columns
        Y0 = Y.copy(); Y0[:, 0] = 2.5
        assert status(e, Y0, C) == BA                                                    # yy = 0
        for v in (0.5, np.inf, np.nan):
            assert status(e, Y, C, max_vif=v) == BA
        Gb = G.copy(); Gb[17, 9] = 3
        load(e, Gb)
        with pytest.raises(GpcaError) as ei:
            e.assoc_linear(Y, C)
        assert ei.value.status == _lib.GPCA_ERR_INVALID_GENOTYPE and "row 17" in str(ei.value)
        assert np.isfinite(e.assoc_linear(Y, C, rows=(0, 17))["t"]).all()                # a band that does not read the row
    # (GPCA_ERR_OOM needs a band whose workspace exceeds the free memory of the card: no shape a quick test can hold reaches it)
    with gpca.GpcaEngine() as e:                                                         # a streamed handle
        e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), M, N, panel_rows=256, ring_slots=2, fused=False)
        e.snp_stats(gpca.QcConfig.none())
        with pytest.raises(GpcaError) as ei:
            e.assoc_linear(Y, C)
        assert ei.value.status == _lib.GPCA_ERR_STATE and "panel" in str(ei.value)
    with gpca.GpcaEngine() as e:                                                         # a hooked (row-sharded) handle
        e.upload_genotypes_i8(G[:20].copy())
        e.set_allreduce_hook(lambda buf: None, 2, 0, 0)
        e.set_standardization(np.ones(20, np.float32), np.ones(20, np.float32), np.ones(20, np.uint8))
        with pytest.raises(GpcaError) as ei:
            e.assoc_linear(Y, C)
        assert ei.value.status == _lib.GPCA_ERR_STATE and "shard" in str(ei.value)


# ------------------------------------------------------------------------------------------------ what it is for
def cohort(seed=7, N=600, K=3000, fst=0.1):
    rng = np.random.default_rng(seed)
    pop = (np.arange(N) >= N // 2).astype(np.int64)
    anc = rng.uniform(0.1, 0.9, K)
    a, b = anc * (1 - fst) / fst, (1 - anc) * (1 - fst) / fst
    p = np.stack([rng.beta(a, b), rng.beta(a, b)], 1)[:, pop]
    G = ((rng.random((K, N)) < p).astype(np.int8) + (rng.random((K, N)) < p).astype(np.int8))
    causal = K // 2
    y = 1.0 * pop + 0.5 * G[causal] + rng.standard_normal(N)
    Z = G - G.mean(1, keepdims=True)
    sd = Z.std(1); ok = sd > 0
    u, _, _ = np.linalg.svd((Z[ok] / sd[ok, None]).T, full_matrices=False)
    return G, y.reshape(N, 1), u[:, :1].copy(), causal


def cohort_figures(t, causal):
    t2 = t[:, 0] ** 2
    null = np.delete(t2, causal)
    null = null[np.isfinite(null)]
    return np.median(null) / 0.454936, t2[causal], null.max()


def check_cohort(lam1, tc, tmax, lam0):
    assert abs(lam1 - 1.0) <= 0.1
    assert tc > tmax
    assert lam0 >= 3.0


def cohort_restatement():
    G, y, pc, causal = cohort()
    out = []
    for C in (pc, np.zeros((len(y), 0))):
        inc = np.ones(len(y), np.uint8)
        B, yy, df, kappa = design(y, C, inc)
        ref = restate(G, B, inc, kappa, C.shape[1])
        out.append(cohort_figures(finish(G @ B, ref["nobs"], ref["s1"], ref["s2"], yy, df, 1)["t"], causal))
    return out


def test_pc_covariate_removes_inflation():
    G, y, pc, causal = cohort()
    with gpca.GpcaEngine() as e:
        load(e, G)
        lam1, tc, tmax = cohort_figures(e.assoc_linear(y, pc)["t"], causal)
        lam0, _, _ = cohort_figures(e.assoc_linear(y)["t"], causal)
    print("lambda with PC 1", lam1, "causal t^2", tc, "largest null t^2", tmax, "lambda without", lam0)
    check_cohort(lam1, tc, tmax, lam0)
