"""gpca_assoc_logistic_spa: the logistic score scan with the saddle-point correction (assoc_spa.hip, gpca_assoc_score.cpp; include/gpca.h
section a14), through the C ABI.

The reference is the numpy f64 restatement of tests/test_assoc_spa_host.py (spa_reference), fed per item (row, trait) with what the
device itself leaves: U and a_0 .. a_Pc of its ua, the flip of its rowinfo, z of its stats; with the genotypes; and with mu and
Z = X L^-T rebuilt here from gpca_logistic_null (the function the call runs inside: the same mu to the bit) and numpy's Cholesky:
    x~ = the operand (2 - g on a flipped row) where observed and included, xbar where missing and included;  g~ = x~ - Z a over S.
The bars are spa_bars of the host test (derived in its docstring) with its input-error term dg, the reconstruction of g~:
    dg = 8 (Pc + 3) kappa e max_n sum_j |a_j Z_nj|     (the engine's L against numpy's: 8 (Pc + 3) kappa e per column of Z, kappa = the
                                                        condition number of X^T W X; the bound tests/test_gpu_assoc_score.py uses)
       + (Pc + 3) e max_n (|x~_n| + sum_j |a_j Z_nj|)  (the Pc + 1 products and additions of the dot product and the subtraction).
The flag |z| >= spa_z is decided on the device's own z, so it is exact.  An item is skipped only where the restatement stands within
its summation error of the support rule (near_decision); at most 2 % of the items of a case may be.

Shapes: 130 kept rows (a 128-row tile plus two), N in {63, 64, 65, 257, 2049} (stage, flush and count-chunk boundaries), (T, Pc) in
{(1, 0), (2, 3), (1, 61)}, the last from N = 257 on; int8 and 2-bit storage; spa_z = 0.5.  The inputs are those of
tests/test_gpu_assoc_score.py (missing calls, excluded samples with extreme values, a flipped row, an all-missing row, a monomorphic
row, a row collinear with a covariate) with traits at a case rate near 0.1.  One exception, stated: (1, 61) at N = 257 takes a case
rate of 0.4, because two dozen cases are separated by 61 covariates and the null fit then refuses the trait.
Status 2 is not constructible through the device at these shapes: it needs a root rule that fails or a tail of the wrong sign, which
the host test builds from |U| = 1e-200 and from a target one ulp inside the support; a kept row cannot carry either with |z| >= 0.5.
Every case asserts that the statuses 0 and 1 occur, and from N = 64 on (where the inputs hold the special rows) the NaN rows.

spa_z = +inf: every status is 0 and -log10 p is the host's gpca_normal_log10p(z) within 16 e max(value, 1): the device's erf, erfc,
log and log1p are each within a few ulp of the host's (HIP documents at most 5), and -log10 p = -ln(erfc) / ln 10 carries those as
absolute errors of the logarithm."""
import math

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from genomic_pca_amd._lib import GpcaError

from test_assoc_spa_host import EPS, calibration_rows, exact_log10p, near_decision, spa_bars, spa_reference
from test_gpu_assoc_score import STORES, VIF, design, load, make_inputs, panel, restate, same

pytestmark = pytest.mark.gpu

M_ROWS = 130
NS = [63, 64, 65, 257, 2049]
TPS = [(1, 0), (2, 3), (1, 61)]
CASES = [(N, T, Pc) for N in NS for T, Pc in TPS if Pc < 61 or N >= 257]
WORST = {"zeta": 0.0, "log10p": 0.0}


def inputs(N, T, Pc, seed=None):
    """make_inputs of the score scan's test with traits at a case rate near 0.1 (0.4 for Pc = 61 at N = 257: module docstring)"""
    seed = 900 + N + Pc if seed is None else seed
    G, Y, C, inc, special = make_inputs(M_ROWS, N, T, Pc, seed=seed, miss=0.03)
    rng = np.random.default_rng(seed + 1)
    rate = 0.4 if (Pc == 61 and N < 1024) else 0.1
    s = inc == 1
    Yn = (rng.random((N, T)) < rate).astype(np.float64)
    for t in range(T):                                  # at least three cases among the included samples
        idx = np.flatnonzero(s)
        Yn[idx[t:t + 3], t] = 1.0
    Yn[~s] = 1e30
    return G, Yn, C, inc, special


def rebuild(Y, C, inc):
    """per trait: mu [N] (the engine's), Z [N][Pc + 1] = X L^-T (0 outside S), kappa"""
    s = inc.astype(bool)
    X = design(C, inc)
    out = []
    for t in range(Y.shape[1]):
        mu = gpca.GpcaEngine.logistic_null(Y[:, t], C, inc)[1]
        w = mu[s] * (1.0 - mu[s])
        H = X.T @ (w[:, None] * X)
        L = np.linalg.cholesky(H)
        Z = np.zeros((Y.shape[0], X.shape[1]))
        Z[s] = np.linalg.solve(L, X.T).T
        out.append((mu, Z, float(np.linalg.cond(H))))
    return out


def operand(G, inc, flipped):
    """x~ of every row without the mean, the mask of the imputed calls, xbar"""
    s = inc.astype(bool)
    o = (G != -127) & s[None, :]
    ms = (G == -127) & s[None, :]
    g = np.where(o, G, 0).astype(np.float64)
    x = np.where(o, np.where(flipped[:, None] > 0, 2.0 - g, g), 0.0)
    with np.errstate(all="ignore"):
        xbar = x.sum(1) / o.sum(1)
    return x, ms, xbar


def check_against_restatement(r, G, inc, nulls, spa_z, Pc):
    """every item of the device's result r against spa_reference; returns (items, skipped)"""
    s = inc.astype(bool)
    x, ms, xbar = operand(G, inc, r["flipped"])
    K, T = r["z"].shape
    items = skipped = 0
    for t in range(T):
        mu, Z, kappa = nulls[t]
        for i in range(K):
            z = r["z"][i, t]
            lp, st, zeta = r["log10p"][i, t], int(r["spa_status"][i, t]), r["zeta"][i, t]
            items += 1
            if z != z:
                assert lp != lp and st == 0 and np.all(np.isnan(zeta)), (i, t)
                continue
            normal = gpca.GpcaEngine.normal_log10p(z)
            Uv, a = r["ua"][i, t, 0], r["ua"][i, t, 2:]
            if not (abs(z) >= spa_z and Uv != 0.0):
                assert st == 0 and np.all(np.isnan(zeta)) and abs(lp - normal) <= 16 * EPS * max(normal, 1.0), (i, t, lp, normal)
                continue
            xt = x[i] + np.where(ms[i], xbar[i], 0.0)
            az = np.abs(Z * a[None, :]).sum(1)
            gt = np.where(s, xt - Z @ a, 0.0)
            dg = 8 * (Pc + 3) * kappa * EPS * float(az.max()) + (Pc + 3) * EPS * float((np.abs(xt) + az).max())
            ref = spa_reference(gt[s], mu[s], Uv, normal=normal)
            if near_decision(gt[s], mu[s], Uv, ref, dg):
                skipped += 1
                continue
            assert st == ref["status"], (i, t, st, ref["status"], zeta, ref["zeta"])
            if st != 1:
                assert abs(lp - normal) <= 16 * EPS * max(normal, 1.0)
                continue
            bz, bp = spa_bars(gt[s], mu[s], ref, dg)
            for side in range(2):
                if math.isinf(ref["zeta"][side]):
                    assert zeta[side] == ref["zeta"][side], (i, t, side)
                    continue
                d = abs(zeta[side] - ref["zeta"][side])
                WORST["zeta"] = max(WORST["zeta"], d / bz[side])
                assert d <= bz[side], (i, t, side, zeta, ref["zeta"], bz)
            if math.isinf(ref["log10p"]):
                assert lp == ref["log10p"]
                continue
            d = abs(lp - ref["log10p"])
            WORST["log10p"] = max(WORST["log10p"], d / bp)
            assert d <= bp, (i, t, lp, ref["log10p"], bp)
    return items, skipped


# ------------------------------------------------------------------------------------------------ 1. the edge shapes
@pytest.mark.parametrize("N,T,Pc", CASES)
def test_spa_at_edge_shapes(N, T, Pc):
    G, Y, C, inc, special = inputs(N, T, Pc)
    nulls = rebuild(Y, C, inc)
    res = {}
    for store in ("int8", "2bit"):
        with gpca.GpcaEngine(storage=STORES[store]) as e:
            load(e, G)
            res[store] = e.assoc_logistic_spa(Y, C, include=inc, max_vif=VIF, spa_z=0.5, ua=True)
    r = res["int8"]
    for k, v in r.items():                              # int8 and 2-bit residency: the same bits
        assert same(v, res["2bit"][k]), k
    assert r["log10p"].shape == (M_ROWS, T) and r["zeta"].shape == (M_ROWS, T, 2)
    items, skipped = check_against_restatement(r, G, inc, nulls, 0.5, Pc)
    st = r["spa_status"]
    print(f"N={N} T={T} Pc={Pc}: {items} items, status 0/1/2: {int((st == 0).sum())}/{int((st == 1).sum())}/{int((st == 2).sum())}, "
          f"NaN {int(np.isnan(r['z']).sum())}, skipped {skipped}; worst / bar so far: zeta {WORST['zeta']:.3g}, log10p {WORST['log10p']:.3g}")
    assert skipped <= 0.02 * items
    assert (st == 1).sum() > 0.3 * items                # spa_z = 0.5: the correction runs on most items
    finite = ~np.isnan(r["z"])
    assert (st[finite] == 0).any() and np.all(st[~finite] == 0)          # status 0 among the tested items; 1 above; the NaN rows below
    if special:
        assert np.all(np.isnan(r["log10p"][2])) and np.all(np.isnan(r["log10p"][M_ROWS // 2]))     # monomorphic; no observed call
        assert r["flipped"][0] == 1.0 and np.isfinite(r["z"][0]).all()                              # the flipped row is tested, and ...
        assert np.array_equal(r["spa_status"][0] == 1, np.abs(r["z"][0]) >= 0.5)                    # ... corrected from the cutoff on


# ------------------------------------------------------------------------------------------------ 2. - 4. cutoffs, pass-through, bits
def test_cutoffs_passthrough_bands_and_storage_bits():
    N, T, Pc = 257, 2, 3
    G, Y, C, inc, _ = inputs(N, T, Pc)
    nulls = rebuild(Y, C, inc)
    out = {}
    for name, store, prec in (("int8", _lib.STORE_INT8, _lib.PREC_I8_EXACT), ("2bit", _lib.STORE_2BIT, _lib.PREC_I8_EXACT),
                              ("f32", _lib.STORE_INT8, _lib.PREC_F32_MFMA)):
        with gpca.GpcaEngine(storage=store, precision=prec) as e:
            load(e, G)
            out[name] = e.assoc_logistic_spa(Y, C, include=inc, max_vif=VIF, ua=True)                  # spa_z = 2, the default
            if name != "int8":
                continue
            score = e.assoc_logistic_score(Y, C, include=inc, max_vif=VIF, ua=True)
            off = e.assoc_logistic_spa(Y, C, include=inc, max_vif=VIF, spa_z=float("inf"), ua=True)
            bands = [e.assoc_logistic_spa(Y, C, include=inc, max_vif=VIF, rows=b, ua=True) for b in ((0, 1), (1, 129), (129, 130), (7, 7))]
    r = out["int8"]
    # pass-through: stats, ua and rowinfo carry the bits of gpca_assoc_logistic_score, at either cutoff
    for k, v in score.items():
        assert same(v, r[k]) and same(v, off[k]), k
    # spa_z = +inf: nothing is corrected, the value is the host's normal one
    assert np.all(off["spa_status"] == 0) and np.all(np.isnan(off["zeta"]))
    for i in range(M_ROWS):
        for t in range(T):
            z, lp = off["z"][i, t], off["log10p"][i, t]
            if z != z:
                assert lp != lp
            else:
                want = gpca.GpcaEngine.normal_log10p(z)
                assert abs(lp - want) <= 16 * EPS * max(want, 1.0), (i, t, lp, want)
    # spa_z = 2: the items at or above the cutoff are corrected, held to the restatement; the others keep the normal value
    items, skipped = check_against_restatement(r, G, inc, nulls, 2.0, Pc)
    flagged = np.abs(r["z"]) >= 2.0
    assert flagged.any() and skipped <= 0.02 * items
    assert np.all(r["spa_status"][flagged] >= 1) and np.all(r["spa_status"][~flagged] == 0)
    assert same(r["log10p"][~flagged], off["log10p"][~flagged])
    # a band is the full call's rows, bit for bit; so are 2-bit residency and an f32-MFMA handle
    for (a, b), band in zip(((0, 1), (1, 129), (129, 130), (7, 7)), bands):
        for k, v in band.items():
            assert v.shape[0] == b - a and same(v, r[k][a:b]), (a, b, k)
    for name in ("2bit", "f32"):
        for k, v in out[name].items():
            assert same(v, r[k]), (name, k)


# ------------------------------------------------------------------------------------------------ 5. flip invariance
def test_flip_invariance():
    """Every row recoded as 2 - g (missing calls kept).  The operand is coded by the minor allele, so a row whose s1 differs from
    n_obs changes its flipped flag and keeps its operand: log10p and zeta keep their bits.  Row 3 has s1 = n_obs (flipped in neither
    coding): its operand is recoded, U changes sign, the tails trade places: zeta+ -> -zeta-, zeta- -> -zeta+.  The two runs of such
    a row start from two different f32 passes: their U and a_j differ by up to the sum of the two ua bars of
    tests/test_gpu_assoc_score.py (restate), so the bar is spa_bars with du = that sum for U and dg widened by max_n sum_j d a_j
    |Z_nj|, taken twice (once per run)."""
    N, T, Pc = 257, 2, 3
    G, Y, C, inc, special = inputs(N, T, Pc)
    assert special
    G2 = np.where(G == -127, G, 2 - G).astype(np.int8)
    nulls = rebuild(Y, C, inc)
    Bs, kappas = panel(Y, C, inc, np.stack([n[0] for n in nulls], 1))
    uabar = restate(G, Bs, kappas, inc, Pc)["bar"] + restate(G2, Bs, kappas, inc, Pc)["bar"]
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        load(e, G)
        a = e.assoc_logistic_spa(Y, C, include=inc, max_vif=VIF, spa_z=0.5, ua=True)
        load(e, G2)
        b = e.assoc_logistic_spa(Y, C, include=inc, max_vif=VIF, spa_z=0.5, ua=True)
    tie = a["flipped"] == b["flipped"]
    live = ~np.isnan(a["z"][:, 0])
    assert tie[3] and live[3] and np.all(a["flipped"][~tie & live] + b["flipped"][~tie & live] == 1.0)
    assert same(a["log10p"][~tie], b["log10p"][~tie]) and same(a["zeta"][~tie], b["zeta"][~tie]) and same(a["z"][~tie], -b["z"][~tie])
    s = inc.astype(bool)
    xa, msa, xbara = operand(G, inc, a["flipped"])
    for t in range(T):
        mu, Z, kappa = nulls[t]
        for i in np.flatnonzero(tie & live):
            if a["spa_status"][i, t] != 1 or b["spa_status"][i, t] != 1:
                continue
            xt = xa[i] + np.where(msa[i], xbara[i], 0.0)
            coef = a["ua"][i, t, 2:]
            az = np.abs(Z * coef[None, :]).sum(1)
            gt = np.where(s, xt - Z @ coef, 0.0)
            dg = 8 * (Pc + 3) * kappa * EPS * float(az.max()) + (Pc + 3) * EPS * float((np.abs(xt) + az).max())
            dg += float((np.abs(Z) @ uabar[i, t, 2:]).max())
            ref = spa_reference(gt[s], mu[s], a["ua"][i, t, 0], normal=0.0)
            bz, bp = spa_bars(gt[s], mu[s], ref, dg, du=float(uabar[i, t, 0]))
            print(f"row {i} trait {t}: |d log10p| {abs(a['log10p'][i, t] - b['log10p'][i, t]):.3g} of {2 * bp:.3g}")
            assert abs(a["log10p"][i, t] - b["log10p"][i, t]) <= 2 * bp
            for side in range(2):
                za, zb = a["zeta"][i, t, side], -b["zeta"][i, t, 1 - side]
                assert za == zb or abs(za - zb) <= 2 * bz[side], (i, t, side, za, zb)


# ------------------------------------------------------------------------------------------------ 6. calibration through the device
def test_calibration_through_the_device():
    rows = calibration_rows()
    G = np.stack([x for x, _ in rows]).astype(np.int8)
    y = rows[0][1]
    assert all(np.array_equal(y.sum(), yy.sum()) for _, yy in rows)
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        load(e, G)
        for i, (x, yy) in enumerate(rows):
            r = e.assoc_logistic_spa(yy, None, rows=(i, i + 1))
            exact = exact_log10p(x, yy)[0]
            normal = gpca.GpcaEngine.normal_log10p(r["z"][0, 0])
            print(f"row {i}: z {r['z'][0, 0]:.2f}  exact {exact:.3f}  device SPA {r['log10p'][0, 0]:.3f}  normal {normal:.2f}")
            assert r["spa_status"][0, 0] == 1 and abs(r["log10p"][0, 0] - exact) <= 0.25 and abs(normal - exact) > 3.0


# ------------------------------------------------------------------------------------------------ 7. errors
def test_errors():
    import ctypes as C
    N, T, Pc = 65, 1, 0
    G, Y, Cm, inc, _ = inputs(N, T, Pc)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    BA, ST = _lib.GPCA_ERR_BAD_ARG, _lib.GPCA_ERR_STATE
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        load(e, G)
        for bad in (0.49, 0.0, -1.0, float("nan"), float("-inf")):
            with pytest.raises(GpcaError) as ei:
                e.assoc_logistic_spa(Y, None, include=inc, spa_z=bad)
            assert ei.value.status == BA and "spa_z" in ei.value.message
        for good in (0.5, float("inf")):
            e.assoc_logistic_spa(Y, None, include=inc, spa_z=good)
        Yv, stats = np.ascontiguousarray(Y), np.zeros((M_ROWS, 1, 5))
        lib = _lib.load()
        assert lib.gpca_assoc_logistic_spa(e._h, vp(Yv), 1, None, 0, vp(inc), 50.0, 2.0, 0, M_ROWS, vp(stats), None, None, None) == BA   # NULL spa
        spa = np.zeros((M_ROWS, 1, 4))
        assert lib.gpca_assoc_logistic_spa(e._h, vp(Yv), 1, None, 0, vp(inc), 50.0, 2.0, 0, M_ROWS, None, vp(spa), None, None) == 0      # spa alone
        assert lib.gpca_assoc_logistic_spa(None, vp(Yv), 1, None, 0, vp(inc), 50.0, 2.0, 0, M_ROWS, None, vp(spa), None, None) == BA
        for kw in (dict(max_vif=0.5), dict(rows=(0, M_ROWS + 1))):                                  # the score call's refusals hold
            with pytest.raises(GpcaError) as ei:
                e.assoc_logistic_spa(Y, None, include=inc, **kw)
            assert ei.value.status == BA
        with pytest.raises(GpcaError) as ei:
            e.assoc_logistic_spa(np.ones((N, 1)), None, include=inc)                               # one class
        assert ei.value.status == BA
    with gpca.GpcaEngine() as e:                                                         # a streamed handle
        e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), M_ROWS, N, panel_rows=256, ring_slots=2, fused=False)
        e.snp_stats(gpca.QcConfig.none())
        with pytest.raises(GpcaError) as ei:
            e.assoc_logistic_spa(Y, None, include=inc)
        assert ei.value.status == ST and "gpca_assoc_logistic_spa" in ei.value.message and "panel" in ei.value.message
    with gpca.GpcaEngine() as e:                                                         # a hooked (row-sharded) handle
        e.upload_genotypes_i8(G[:20].copy())
        e.set_allreduce_hook(lambda buf: None, 2, 0, 0)
        e.set_standardization(np.ones(20, np.float32), np.ones(20, np.float32), np.ones(20, np.uint8))
        with pytest.raises(GpcaError) as ei:
            e.assoc_logistic_spa(Y, None, include=inc)
        assert ei.value.status == ST and "shard" in ei.value.message
