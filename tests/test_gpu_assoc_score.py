"""gpca_assoc_logistic_score: the logistic score scan of the kept rows (assoc_score.hip, gpca_assoc_score.cpp), through the C ABI.

The definitions every layer implements, restated in numpy f64 (``panel``, ``restate``, ``finish``).  K kept rows in PCA-SNP order, N
samples, T case / control traits Y, Pc covariates C, an include mask; g = the call, S = the included samples.
  1. gpca_logistic_null gives mu of every trait (tests/test_assoc_score_host.py holds it to its own bars; this module builds its
     panel from the engine's mu, so the fit's tolerance does not enter the bars below).
  2. X = (1, C centred over S and scaled to unit norm); per trait r = y - mu, w = mu (1 - mu), A = W X L^-T with X^T W X = L L^T
     (numpy's Cholesky), 0 outside S: Pc + 3 columns.
  3. o = [observed and in S], m = [missing and in S]; n_obs = sum o, s1 = sum g o, s2 = sum g^2 o; a row is flipped iff s1 > n_obs; the
     operand x = g o, or (2 - g) o on a flipped row; d_c = sum x B_c, e_c = sum m B_c, q = sum x^2 w.  The device multiplies the f32
     roundings of the columns by x, m and x^2 as f32 (0, 1, 2, 4: exact products) and sums them in f32 over flush groups of F = 256
     samples (kAscFlush, plan_math.h) counted from sample 0; the groups are added in f64.
  4. xbar = (s1 or 2 n_obs - s1) / n_obs; U = d[r] + xbar e[r], a_j = d[A_j] + xbar e[A_j], gwg = q + xbar^2 e[w]; vw = gwg - a_0^2,
     V = vw - sum_{j >= 1} a_j^2 (j ascending), s = -1 on a flipped row; beta = s U / V, se = 1 / sqrt(V), z = s U / sqrt(V);
     a1_freq = (s1 / n_obs) / 2, xx = s2 - s1 (s1 / n_obs); NaN when n_obs = 0, xx <= 0, !(V > 0) or V max_vif < vw.

The bars (u = 2^-24, e = 2^-53, F = 256), the derivation of tests/test_gpu_assoc.py with this scan's operands:
  ua: a column rounds once to f32 (u |B|; its products with 0, 1, 2, 4 are then exact), every partial sum of a flush group of at most
    F terms rounds once, and a v_mfma_f32_32x32x2_f32 that rounds the sum of its two products costs one more: (F + 3) u S covers the
    first order F + 2 and the second.  The f64 side, counted: N / F + 1 additions of groups, the division, the product with xbar and
    the last addition, (N / F + 4) e S.  S = sum |x B| + xbar sum_miss |B| for U and each a_j, S = sum x^2 w + xbar^2 sum_miss w for
    gwg.  The engine's L against numpy's, and its standardised X against this module's: at most 8 (Pc + 3) kappa e per column
    (kappa = the condition number of X^T W X, computed here), times |B_j|_2 times sum_n |x~_n| (x~ = x with the mean imputed).
    (F + 3) u N = 0.0158 < 1 / 2 at N = 1 025 (asserted): the bar stays under half an average term, and every shape asserts that
    leaving one included sample out of the restatement breaks it somewhere.
  n_obs and flipped are exact; a1_freq and xx are the f64 formulas of integers, bit for bit.
  stats from the device's own ua in f64 with the order of step 4: one rounding per operation on either side; vw and V lose at most a
    factor gwg / V to cancellation and the sums have Pc + 1 products: 4 (Pc + 3) (gwg / V) e relative, computed per row (for vw and V
    themselves that is 4 (Pc + 3) e gwg absolute, which also holds where V is not positive).
  End to end against the direct f64 formula in A1 coding, V = g~^T W g~ - g~^T W X (X^T W X)^-1 X^T W g~ (numpy.linalg.solve), U =
    g~^T (y - mu), z = U / sqrt(V): first order from the ua bars, d V = d gwg + sum_j 2 |a_j| d a_j, d z = d U / sqrt(V) + |z| d V /
    (2 V), each doubled for the second order, plus the formula's own error: 64 kappa^2 e of the larger term it subtracts (g~^T W g~)
    for V, and for z that over 2 V plus 64 kappa^2 e, times |z|.
  Flip invariance: a matrix and its 2 - g recoding (missing calls kept) give V within the sum of the two V bars, and beta and z
    negated within the sum of the two propagated bars.
Every case prints the largest fraction of the ua bar it observes ("ua: max err / bar").

What it is for (test_pc_covariate_removes_inflation): N = 600 (two populations of 300 at F_ST = 0.1, Balding-Nichols), K = 3 000 SNPs,
logit P(case) = -0.7 + 1.4 [population 1] + 0.8 (g_causal - mean), causal SNP = row 1 500; PC 1 = the first left singular vector of the
standardised genotypes (numpy SVD); lambda = median z^2 over the other SNPs / 0.4549 (the chi^2_1 median).  Seed 6, chosen among
seeds 1 .. 12 as one where the f64 restatement alone (cohort_restatement) clears every bound by a factor of at least 2:
  Pc = 1: lambda = 1.0126 (bound |lambda - 1| <= 0.1: measured 0.0126, a factor 7.9), and the causal SNP is the top hit: z^2 = 35.45
  against the largest null 12.65 (bound: ratio > 1, measured 2.80);  Pc = 0: lambda = 7.38 (bound >= 3: a factor 2.46).
  On the 200 leading SNPs the score z lies within 0.0315 of the Wald z of a full logistic fit per SNP (numpy IRLS), inside the 0.05
  the method is expected to keep at this sample size; the device's figure is asserted at twice the restatement's, 0.063."""
import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from genomic_pca_amd._lib import GpcaError

pytestmark = pytest.mark.gpu

STORES = {"int8": _lib.STORE_INT8, "2bit": _lib.STORE_2BIT}
U = 2.0 ** -24
EPS = 2.0 ** -53
F_ASC = 256           # kAscFlush (plan_math.h; restated in the header comment of assoc_score.hip)
C_ASC = 3.0           # module docstring
VIF = 50.0
assert (F_ASC + C_ASC) * U * 1025 < 0.5
NS = [4, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
KS = [1, 127, 128, 129, 4097]
TPS = [(1, 0), (10, 0), (8, 1), (1, 29), (1, 30), (2, 29), (16, 1), (21, 0), (1, 61)]
assert [t * (p + 3) for t, p in TPS] == [3, 30, 32, 32, 33, 64, 64, 63, 64]

COHORT_SEED = 6       # module docstring
WALD_GAP = 0.0315     # max |score z - Wald z| over the 200 leading SNPs, the f64 restatement alone (module docstring)


# ------------------------------------------------------------------------------------------------ inputs
def make_inputs(M, N, T, Pc, seed, miss):
    """two populations; about one sample in ten is excluded when N allows, and the excluded samples hold missing calls and extreme
    trait and covariate values; sample N // 3 (included) has every call missing; with miss = 0 no other call of an included sample
    is missing, so the ballot stays quiet outside that sample's group.  From 64 samples and 6 rows on: row 0 has an A1 frequency
    of 0.9 (one call in five is 1, the others 2: it flips), row 1 is collinear with covariate 0 (the VIF rule; where Pc > 0), row 2
    is monomorphic among the included samples, row 3 has s1 = n_obs exactly (it does not flip), row M // 2 has no observed call."""
    rng = np.random.default_rng(seed)
    pop = np.arange(N) % 2
    p = np.stack([rng.uniform(0.1, 0.9, M), rng.uniform(0.1, 0.9, M)], 1)[:, pop]
    special = N >= 64 and M >= 6
    G = (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)
    inc = np.ones(N, np.uint8)
    if N >= 64:
        inc[rng.random(N) < 0.1] = 0
        inc[N // 3] = 1
    if miss > 0:
        G[rng.random((M, N)) < miss] = -127
    G[:, inc == 0] = -127
    if N >= 8:
        G[:, N // 3] = -127
    C = rng.standard_normal((N, Pc))
    n = np.arange(N)
    Y = (rng.random((N, T)) < 1.0 / (1.0 + np.exp(-(0.8 * (n % 2) - 0.4)))[:, None]).astype(np.float64)
    if N == 4:
        Y[:] = np.array([0.0, 1.0, 0.0, 1.0])[:, None]
    s = inc == 1
    if special:
        o0 = np.flatnonzero(s & (G[0] != -127))
        G[0, o0] = np.where(np.arange(len(o0)) % 5 == 0, 1, 2)
        G[M // 2, :] = -127
        G[2, s & (G[2] != -127)] = 2
        o = np.flatnonzero(s & (G[3] != -127))
        G[3, o] = np.where(np.arange(len(o)) % 2 == 0, 0, 2)
        if len(o) % 2:
            G[3, o[-1]] = 1
        if Pc:
            o1 = (G[1] != -127) & s
            C[:, 0] = np.where(G[1] == -127, G[1][o1].mean(), G[1]) + 1e-7 * C[:, 0]
    Y[inc == 0] = 1e30
    C[inc == 0] = -1e30
    return G, Y, C, inc, special


# ------------------------------------------------------------------------------------------------ the f64 restatement
def design(C, inc):
    s = np.asarray(inc).astype(bool)
    Cc = C[s] - C[s].mean(0)
    Cc = Cc / np.sqrt((Cc ** 2).sum(0))
    return np.hstack([np.ones((int(s.sum()), 1)), Cc])


def null_mu(Y, C, inc):
    """the engine's own fit: mu [N][T]"""
    return np.stack([gpca.GpcaEngine.logistic_null(Y[:, t], C, inc)[1] for t in range(Y.shape[1])], 1)


def panel(Y, C, inc, mu):
    """per trait t: B_t [N][Pc + 3] = r, w, A_0 .. A_Pc (ua's order), 0 outside S; kappa_t of X^T W X"""
    s = np.asarray(inc).astype(bool)
    X = design(C, inc)
    N, T = Y.shape
    out, kappas = [], []
    for t in range(T):
        m = mu[s, t]
        w = m * (1.0 - m)
        H = X.T @ (w[:, None] * X)
        L = np.linalg.cholesky(H)
        A = np.linalg.solve(L, (w[:, None] * X).T).T            # A L^T = W X
        B = np.zeros((N, X.shape[1] + 2))
        B[s, 0] = Y[s, t] - m
        B[s, 1] = w
        B[s, 2:] = A
        out.append(B)
        kappas.append(np.linalg.cond(H))
    return out, kappas


def restate(Gk, Bs, kappas, inc, Pc, drop=None):
    s = np.asarray(inc).astype(bool)
    N = Gk.shape[1]
    o = (Gk != -127) & s
    ms = ((Gk == -127) & s).astype(np.float64)
    g = np.where(o, Gk, 0).astype(np.float64)
    nobs, s1, s2 = o.sum(1), g.sum(1), (g * g).sum(1)
    flip = s1 > nobs
    x = np.where(o, np.where(flip[:, None], 2.0 - g, g), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        xbar = np.where(flip, 2.0 * nobs - s1, s1) / nobs
    xb0 = np.where(nobs > 0, xbar, 0.0)
    xd, md = x, ms
    if drop is not None:
        xd, md = x.copy(), ms.copy(); xd[:, drop] = 0.0; md[:, drop] = 0.0
    xt = (x + xb0[:, None] * ms).sum(1)
    K, T = Gk.shape[0], len(Bs)
    ua, bar = np.zeros((K, T, Pc + 3)), np.zeros((K, T, Pc + 3))
    f = (F_ASC + C_ASC) * U + (N / F_ASC + 4) * EPS
    for t, B in enumerate(Bs):
        chol = 8 * (Pc + 3) * kappas[t] * EPS * xt[:, None] * np.sqrt((B ** 2).sum(0))[None, :]
        with np.errstate(invalid="ignore"):
            v = xd @ B + xbar[:, None] * (md @ B)
            v[:, 1] = (xd * xd) @ B[:, 1] + xbar * xbar * (md @ B[:, 1])
        S = xd @ np.abs(B) + xb0[:, None] * (md @ np.abs(B))
        S[:, 1] = (xd * xd) @ B[:, 1] + xb0 * xb0 * (md @ B[:, 1])
        ua[:, t], bar[:, t] = v, f * S + chol
    return dict(nobs=nobs, s1=s1, s2=s2, flip=flip, ua=ua, bar=bar)


def finish(ua, nobs, s1, s2, vif=VIF):
    with np.errstate(all="ignore"):
        flip = s1 > nobs
        mbar = s1 / nobs
        xx = s2 - s1 * mbar
        Uv, gwg, a = ua[:, :, 0], ua[:, :, 1], ua[:, :, 2:]
        vw = gwg - a[:, :, 0] * a[:, :, 0]
        q = np.zeros_like(vw)
        for j in range(1, a.shape[2]):
            q = q + a[:, :, j] * a[:, :, j]
        V = vw - q
        sg = np.where(flip, -1.0, 1.0)[:, None]
        rt = np.sqrt(V)
        beta, se, z = sg * Uv / V, 1.0 / rt, sg * Uv / rt
        dead = ((nobs == 0) | ~(xx > 0))[:, None] | ~(V > 0) | (V * vif < vw)
    beta, se, z = (np.where(dead, np.nan, v) for v in (beta, se, z))
    return dict(a1_freq=mbar / 2, xx=xx, flipped=flip.astype(np.float64), vw=vw, V=V, beta=beta, se=se, z=z)


def direct(Gk, Y, C, inc, mu, rows, t):
    """(U, V, g~^T W g~, kappa) of rows `rows` for trait t by the direct f64 formula in A1 coding"""
    s = np.asarray(inc).astype(bool)
    X = design(C, inc)
    m = mu[s, t]
    w = m * (1.0 - m)
    H = X.T @ (w[:, None] * X)
    out = []
    for k in rows:
        g = Gk[k, s].astype(np.float64)
        ob = g != -127
        gt = np.where(ob, g, g[ob].mean())
        b = X.T @ (w * gt)
        big = gt @ (w * gt)
        out.append((gt @ (Y[s, t] - m), big - b @ np.linalg.solve(H, b), big))
    return np.array(out), np.linalg.cond(H)


def load(e, G, keep=None):
    e.upload_genotypes_i8(G)
    M = G.shape[0]
    e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.ones(M, np.uint8) if keep is None else keep)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def propagate(ua, bar):
    """first-order bars of V, and of z given V > 0, from the ua bars (doubled): d V, d z"""
    Uv, a = ua[..., 0], ua[..., 2:]
    dV = 2 * (bar[..., 1] + np.sum(2 * np.abs(a) * bar[..., 2:], -1))
    with np.errstate(all="ignore"):
        vw = ua[..., 1] - a[..., 0] ** 2
        V = vw - np.sum(a[..., 1:] ** 2, -1)
        dz = 2 * bar[..., 0] / np.sqrt(V) + np.abs(Uv) / np.sqrt(V) * dV / (2 * V)
    return dV, dz


# ------------------------------------------------------------------------------------------------ the edge shapes
def _cases():
    out, i = [], 0
    for N in NS:
        out.append((4097, N, i)); i += 1
    for M in KS[:-1]:
        for N in (257, 1025):
            out.append((M, N, i)); i += 1
    return out


_CASES = _cases()
_REF = {}


def _shape(N, i):
    T, Pc = TPS[i % len(TPS)]
    Pc = min(Pc, N // 8)                               # Pc <= N / 8 is kept
    return T, Pc


def test_every_panel_width_is_covered():
    got = {_shape(N, i) for _, N, i in _CASES}
    assert {tp for tp in TPS} <= got, sorted(set(TPS) - got)


@pytest.mark.parametrize("store", ["int8", "2bit"])
@pytest.mark.parametrize("M,N,i", _CASES)
def test_scan_at_edge_shapes(store, M, N, i):
    T, Pc = _shape(N, i)
    G, Y, C, inc, special = make_inputs(M, N, T, Pc, seed=500 + i, miss=0.03 if i % 2 else 0.0)
    s = inc.astype(bool)
    if i not in _REF:
        mu = null_mu(Y, C, inc)
        Bs, kappas = panel(Y, C, inc, mu)
        ref = restate(G, Bs, kappas, inc, Pc)
        drop = int(np.flatnonzero(s)[np.argmax(((G[:, s] != -127) & (G[:, s] != 0)).sum(0))])
        _REF[i] = (mu, Bs, kappas, ref, restate(G, Bs, kappas, inc, Pc, drop=drop))
    mu, Bs, kappas, ref, dropped = _REF[i]
    if special:                                        # the rows the issue names are in the inputs
        o = (G != -127) & s
        freq = np.where(o, G, 0).sum(1) / np.maximum(o.sum(1), 1) / 2
        assert abs(freq[0] - 0.9) < 0.02 and ref["flip"][0]
        assert ref["s1"][3] == ref["nobs"][3] > 0 and not ref["flip"][3]
        assert ref["nobs"][M // 2] == 0
        assert ref["nobs"][2] > 0 and ref["s2"][2] * ref["nobs"][2] == ref["s1"][2] ** 2
        assert s[N // 3] and np.all(G[:, N // 3] == -127)
        assert np.all(G[:, ~s] == -127) and np.all(Y[~s] == 1e30)
        if Pc:
            assert abs(np.corrcoef(np.where(o[1], G[1], 0)[s & o[1]], C[s & o[1], 0])[0, 1]) > 0.999999
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        load(e, G)
        r = e.assoc_logistic_score(Y, C, include=inc, max_vif=VIF, ua=True)
    K = M
    assert r["ua"].shape == (K, T, Pc + 3) and r["beta"].shape == (K, T)
    # exact outputs
    assert np.array_equal(r["n_obs"], ref["nobs"].astype(np.float64))
    fin0 = finish(ref["ua"], ref["nobs"], ref["s1"], ref["s2"])
    assert same(r["a1_freq"], fin0["a1_freq"]) and same(r["xx"], fin0["xx"]) and same(r["flipped"], fin0["flipped"])
    # ua against the bar
    live = ref["nobs"] > 0
    assert np.all(np.isnan(r["ua"][~live])) and np.all(np.isnan(r["beta"][~live]))
    err = np.abs(r["ua"][live] - ref["ua"][live])
    bar = ref["bar"][live]
    if live.any():
        print("ua: max err / bar", np.max(err / np.maximum(bar, 1e-300)), "kappa", max(kappas))
    assert np.all(err <= bar)
    if live.any():
        assert np.any(np.abs(r["ua"][live] - dropped["ua"][live]) > dropped["bar"][live])
    # the statistics from the device's own ua
    fin = finish(r["ua"], ref["nobs"], ref["s1"], ref["s2"])
    gwg = r["ua"][:, :, 1]
    tol_abs = 4 * (Pc + 3) * EPS * np.abs(gwg)
    for k in ("vw", "V"):
        assert same(np.isnan(r[k]), np.isnan(fin[k])), k
        ok = ~np.isnan(fin[k])
        assert np.all(np.abs(r[k][ok] - fin[k][ok]) <= tol_abs[ok]), k
    with np.errstate(all="ignore"):
        tol_rel = 4 * (Pc + 3) * EPS * np.abs(gwg) / fin["V"]
    for k in ("beta", "se", "z"):
        assert same(np.isnan(r[k]), np.isnan(fin[k])), k
        ok = ~np.isnan(fin[k])
        assert np.all(np.abs(r[k][ok] - fin[k][ok]) <= tol_rel[ok] * np.abs(fin[k][ok])), k
    if special:
        assert np.all(np.isnan(r["z"][2])) and r["xx"][2] == 0.0                  # monomorphic among the included samples
        assert np.all(np.isnan(r["z"][M // 2]))                                   # no observed call
        assert np.isfinite(r["z"][0]).all() and np.isfinite(r["z"][3]).all()
        if Pc:
            assert np.all(np.isnan(r["z"][1]))                                    # collinear with covariate 0: the VIF rule
    # end to end: the direct formula in A1 coding, a spread of rows
    pick = [int(k) for k in np.unique(np.linspace(0, K - 1, 24).astype(int)) if np.isfinite(r["z"][k]).all()]
    dV, dz = propagate(ref["ua"], ref["bar"])
    for t in sorted({0, T - 1}):
        d, kap = direct(G, Y, C, inc, mu, pick, t)
        for (Ur, Vr, big), k in zip(d, pick):
            own = 64 * kap ** 2 * EPS
            V, z = r["V"][k, t], r["z"][k, t]
            assert abs(V - Vr) <= dV[k, t] + own * big, (k, t, V, Vr, dV[k, t])
            zr = Ur / np.sqrt(Vr)
            assert abs(z - zr) <= dz[k, t] + abs(zr) * (own * big / (2 * Vr) + own), (k, t, z, zr, dz[k, t])
    assert pick or not np.isfinite(r["z"]).any()


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
            out[name] = e.assoc_logistic_score(Y, C, include=inc, ua=True)
            if name == "int8":
                bands = [e.assoc_logistic_score(Y, C, include=inc, ua=True, rows=b) for b in ((0, 1), (1, 130), (130, 131), (131, 640), (640, K), (K, K))]
                G2, Y2, C2 = G.copy(), Y.copy(), C.copy()
                x = inc == 0
                assert x.sum() >= 5
                G2[:, x] = np.random.default_rng(1).integers(0, 3, (M, int(x.sum())))
                Y2[x] = -7.0; C2[x] = 3.0
                load(e, G2, keep)
                out["changed"] = e.assoc_logistic_score(Y2, C2, include=inc, ua=True)
                e.set_sample_mask((np.arange(N) % 2).astype(np.uint8))              # the sample mask is ignored
                out["masked"] = e.assoc_logistic_score(Y2, C2, include=inc, ua=True)
    ref = out["int8"]
    assert np.isfinite(ref["z"]).sum() > K * T // 2
    for k in ref:
        assert same(np.concatenate([b[k] for b in bands]), ref[k]), k
        for other in ("2bit", "f32", "changed", "masked"):
            assert same(out[other][k], ref[k]), (other, k)


def test_flip_invariance():
    M, N, T, Pc = 300, 257, 2, 3
    G, Y, C, inc, _ = make_inputs(M, N, T, Pc, seed=11, miss=0.03)
    Gr = np.where(G == -127, G, 2 - G).astype(np.int8)
    mu = null_mu(Y, C, inc)
    Bs, kappas = panel(Y, C, inc, mu)
    res, bars, refs = [], [], []
    for g in (G, Gr):
        with gpca.GpcaEngine() as e:
            load(e, g)
            res.append(e.assoc_logistic_score(Y, C, include=inc, max_vif=VIF))
        ref = restate(g, Bs, kappas, inc, Pc)
        bars.append(propagate(ref["ua"], ref["bar"]))
        refs.append(ref)
    a, b = res
    ok = np.isfinite(a["z"]) & np.isfinite(b["z"])
    assert ok.sum() > M * T // 2 and same(np.isnan(a["z"]), np.isnan(b["z"]))
    dV, dz = bars[0][0] + bars[1][0], bars[0][1] + bars[1][1]
    assert np.all(np.abs(a["V"] - b["V"])[ok] <= dV[ok])
    assert np.all(np.abs(a["z"] + b["z"])[ok] <= dz[ok])
    with np.errstate(all="ignore"):
        dbeta = dz / np.sqrt(a["V"]) + np.abs(a["beta"]) * dV / a["V"]                # beta = z / sqrt(V)
    assert np.all(np.abs(a["beta"] + b["beta"])[ok] <= 2 * dbeta[ok])
    # a row away from s1 = n_obs is flipped in exactly one of the two, and there the operands, hence the bits of V, are the same
    both = (refs[0]["s1"] != refs[0]["nobs"]) & (refs[0]["nobs"] > 0)
    assert both.sum() > M // 2
    assert np.all((a["flipped"] + b["flipped"])[both] == 1.0)
    assert same(a["V"][both], b["V"][both])


# ------------------------------------------------------------------------------------------------ errors
def test_errors():
    M, N = 40, 50
    rng = np.random.default_rng(3)
    G = rng.integers(0, 3, (M, N)).astype(np.int8)
    Y, C = (rng.random((N, 2)) < 0.5).astype(np.float64), rng.standard_normal((N, 3))
    lib = _lib.load()

    def status(e, *a, **k):
        with pytest.raises(GpcaError) as ei:
            e.assoc_logistic_score(*a, **k)
        return ei.value.status, str(ei.value)

    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(G)
        assert status(e, Y, C)[0] == _lib.GPCA_ERR_STATE                                 # no standardisation
        load(e, G, np.zeros(M, np.uint8))
        assert status(e, Y, C)[0] == _lib.GPCA_ERR_STATE                                 # K = 0
        load(e, G)
        BA = _lib.GPCA_ERR_BAD_ARG
        assert status(e, np.zeros((N, 0)), C)[0] == BA                                   # T = 0
        assert status(e, (rng.random((N, 11)) < 0.5) * 1.0, C)[0] == BA                  # T (Pc + 3) = 66 > 64
        assert np.isfinite(e.assoc_logistic_score((rng.random((N, 10)) < 0.5) * 1.0, C)["V"]).all()      # 60 columns
        for rows in ((-1, 3), (5, 4), (0, M + 1)):
            assert status(e, Y, C, rows=rows)[0] == BA
        vp = lambda a: a.ctypes.data
        assert lib.gpca_assoc_logistic_score(e._h, vp(Y), 2, vp(C), 3, None, 50.0, 0, M, None, None, None) == BA     # all outputs NULL
        Yn = Y.copy(); Yn[7, 1] = np.nan
        st, msg = status(e, Yn, C)
        assert st == BA and "trait 1" in msg                                             # the failure names the trait
        inc = np.ones(N, np.uint8); inc[7] = 0
        assert np.isfinite(e.assoc_logistic_score(Yn, C, include=inc)["V"]).all()        # ... but not on an excluded sample
        Yh = Y.copy(); Yh[3, 0] = 0.5
        assert status(e, Yh, C)[0] == BA                                                 # y outside {0, 1}
        Y1 = Y.copy(); Y1[:, 1] = 1.0
        st, msg = status(e, Y1, C)
        assert st == BA and "trait 1" in msg and "one class" in msg
        Cn = C.copy(); Cn[3, 0] = np.inf
        assert status(e, Y, Cn)[0] == BA
        few = np.zeros(N, np.uint8); few[:4] = 1
        assert status(e, Y, C, include=few)[0] == BA                                     # n - Pc - 1 = 4 - 3 - 1 < 1
        Cc = C.copy(); Cc[:, 1] = 4.0
        assert status(e, Y, Cc)[0] == BA                                                 # a constant column
        Cl = C.copy(); Cl[:, 2] = Cl[:, 0] - 2 * Cl[:, 1]
        assert status(e, Y, Cl)[0] == BA                                                 # collinear columns
        Ys = Y.copy(); Ys[:, 0] = C[:, 0] > 0
        st, msg = status(e, Ys, C)
        assert st == _lib.GPCA_ERR_NOT_CONVERGED and "trait 0" in msg                    # a perfectly separating covariate
        for v in (0.5, np.inf, np.nan):
            assert status(e, Y, C, max_vif=v)[0] == BA
        Gb = G.copy(); Gb[17, 9] = 3
        load(e, Gb)
        st, msg = status(e, Y, C)
        assert st == _lib.GPCA_ERR_INVALID_GENOTYPE and "row 17" in msg
        assert np.isfinite(e.assoc_logistic_score(Y, C, rows=(0, 17))["V"]).all()        # a band that does not read the row
    # (GPCA_ERR_OOM needs a band whose workspace exceeds the free memory of the card: no shape a quick test can hold reaches it)
    with gpca.GpcaEngine() as e:                                                         # a streamed handle
        e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), M, N, panel_rows=256, ring_slots=2, fused=False)
        e.snp_stats(gpca.QcConfig.none())
        st, msg = status(e, Y, C)
        assert st == _lib.GPCA_ERR_STATE and "panel" in msg
    with gpca.GpcaEngine() as e:                                                         # a hooked (row-sharded) handle
        e.upload_genotypes_i8(G[:20].copy())
        e.set_allreduce_hook(lambda buf: None, 2, 0, 0)
        e.set_standardization(np.ones(20, np.float32), np.ones(20, np.float32), np.ones(20, np.uint8))
        st, msg = status(e, Y, C)
        assert st == _lib.GPCA_ERR_STATE and "shard" in msg


# ------------------------------------------------------------------------------------------------ what it is for
def cohort(seed=COHORT_SEED, N=600, K=3000, fst=0.1):
    rng = np.random.default_rng(seed)
    pop = (np.arange(N) >= N // 2).astype(np.int64)
    anc = rng.uniform(0.1, 0.9, K)
    a, b = anc * (1 - fst) / fst, (1 - anc) * (1 - fst) / fst
    p = np.stack([rng.beta(a, b), rng.beta(a, b)], 1)[:, pop]
    G = ((rng.random((K, N)) < p).astype(np.int8) + (rng.random((K, N)) < p).astype(np.int8))
    causal = K // 2
    eta = -0.7 + 1.4 * pop + 0.8 * (G[causal] - G[causal].mean())
    y = (rng.random(N) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    Z = G - G.mean(1, keepdims=True)
    sd = Z.std(1); ok = sd > 0
    u, _, _ = np.linalg.svd((Z[ok] / sd[ok, None]).T, full_matrices=False)
    return G, y.reshape(N, 1), u[:, :1].copy(), causal


def cohort_figures(z, causal):
    z2 = z[:, 0] ** 2
    null = np.delete(z2, causal)
    null = null[np.isfinite(null)]
    return np.median(null) / 0.454936, z2[causal], null.max()


def wald_z(G, y, C, rows):
    """a full logistic fit per SNP (numpy IRLS on (1, C, g)): the Wald z of g"""
    out = []
    N = len(y)
    for k in rows:
        X = np.hstack([np.ones((N, 1)), C, G[k][:, None].astype(np.float64)])
        b = np.zeros(X.shape[1])
        for _ in range(50):
            m = 1.0 / (1.0 + np.exp(-X @ b))
            H = X.T @ ((m * (1 - m))[:, None] * X)
            d = np.linalg.solve(H, X.T @ (y - m))
            b += d
            if np.max(np.abs(d)) < 1e-12:
                break
        m = 1.0 / (1.0 + np.exp(-X @ b))
        cov = np.linalg.inv(X.T @ ((m * (1 - m))[:, None] * X))
        out.append(b[-1] / np.sqrt(cov[-1, -1]))
    return np.array(out)


def cohort_restatement(seed=COHORT_SEED, wald=True):
    G, y, pc, causal = cohort(seed)
    out = []
    inc = np.ones(len(y), np.uint8)
    for C in (pc, np.zeros((len(y), 0))):
        Bs, kappas = panel(y, C, inc, null_mu(y, C, inc))
        ref = restate(G, Bs, kappas, inc, C.shape[1])
        fin = finish(ref["ua"], ref["nobs"], ref["s1"], ref["s2"])
        out.append(cohort_figures(fin["z"], causal))
        if C.shape[1] and wald:
            out.append(float(np.max(np.abs(fin["z"][:200, 0] - wald_z(G, y[:, 0], C, range(200))))))
    return out


def test_pc_covariate_removes_inflation():
    G, y, pc, causal = cohort()
    with gpca.GpcaEngine() as e:
        load(e, G)
        z1 = e.assoc_logistic_score(y, pc)["z"]
        lam1, zc, zmax = cohort_figures(z1, causal)
        lam0, _, _ = cohort_figures(e.assoc_logistic_score(y)["z"], causal)
    gap = float(np.max(np.abs(z1[:200, 0] - wald_z(G, y[:, 0], pc, range(200)))))
    print("lambda with PC 1", lam1, "causal z^2", zc, "largest null z^2", zmax, "lambda without", lam0, "max |score z - Wald z|", gap)
    assert abs(lam1 - 1.0) <= 0.1
    assert lam0 >= 3.0
    assert zc > zmax and int(np.nanargmax(z1[:, 0] ** 2)) == causal
    assert gap <= 2 * WALD_GAP
