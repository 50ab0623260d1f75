"""gpca_assoc_logistic_firth: the logistic score scan with the approximate Firth correction (assoc_firth.hip, gpca_assoc_score.cpp;
include/gpca.h section a15), through the C ABI.

The reference is the numpy f64 restatement of tests/test_assoc_firth_host.py (firth_reference), fed per item (row, trait) as
tests/test_gpu_assoc_spa.py feeds the saddle-point one: U and a_0 .. a_Pc of the device's ua, the flip of its rowinfo, z of its stats,
the genotypes, and mu and Z = X L^-T rebuilt from gpca_logistic_null and numpy's Cholesky.  The bars are firth_bars of the host test
(derived in its docstring) with the input-error term dg of the saddle-point test (the reconstruction of g~).  The flag |z| >= firth_z
is decided on the device's own z, so it is exact.  No item is skipped, and status 2 is not expected: every item with a finite z must
come back corrected.

Shapes: 130 kept rows (a 128-row tile plus two), N in {63, 64, 65, 257, 2049, 8193} (stage, flush and count-chunk boundaries; the last
crosses the 8192-sample staging chunk), (T, Pc) in {(1, 0), (2, 3), (1, 61)}, the last from N = 257 on and there at a case rate of 0.4
(two dozen cases are separated by 61 covariates and the null fit refuses the trait); int8 and 2-bit storage; firth_z = 0, so every
item with a finite z is corrected.  The inputs are those of tests/test_gpu_assoc_spa.py (missing calls, excluded samples with
extreme values, a flipped row with an A1 frequency of 0.9, an all-missing row, a monomorphic row) and three rows more: row 5 a
singleton carried by a case of trait 0, row 6 a singleton carried by a control, row 7 a dozen carriers (fewer at small N) who are
all cases: the score scan's beta = U / V of that row means nothing, Firth's estimate is finite and positive."""
import ctypes as C
import math

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from genomic_pca_amd._lib import GpcaError

from test_assoc_firth_host import CALIBRATION, firth_bars, firth_reference
from test_assoc_spa_host import EPS, calibration_rows
from test_gpu_assoc_score import STORES, VIF, load, panel, restate, same
from test_gpu_assoc_spa import M_ROWS, inputs as spa_inputs, operand, rebuild

pytestmark = pytest.mark.gpu

NS = [63, 64, 65, 257, 2049, 8193]
TPS = [(1, 0), (2, 3), (1, 61)]
CASES = [(N, T, Pc) for N in NS for T, Pc in TPS if Pc < 61 or N >= 257]
WORST = {"beta": 0.0, "log10p": 0.0, "se": 0.0, "D": 0.0, "passes": 0}
BANDS = ((0, 1), (1, 129), (129, 130), (7, 7))
_CACHE = {}


def inputs(N, T, Pc):
    """the saddle-point test's inputs with rows 5, 6, 7 rewritten (module docstring); computed once per shape"""
    if (N, T, Pc) not in _CACHE:
        G, Y, Cm, inc, special = spa_inputs(N, T, Pc)
        s = inc == 1
        obs = s & (np.arange(N) != N // 3)
        cases, ctrls = np.flatnonzero(obs & (Y[:, 0] == 1.0)), np.flatnonzero(obs & (Y[:, 0] == 0.0))
        for row, who in ((5, cases[:1]), (6, ctrls[:1]), (7, cases[:12])):
            G[row, obs] = 0
            G[row, who] = 1
        G[7, cases[0]] = 2
        _CACHE[(N, T, Pc)] = (G, Y, Cm, inc, special, rebuild(Y, Cm, inc))
    return _CACHE[(N, T, Pc)]


def item_inputs(r, x, ms, xbar, s, null, i, t, Pc):
    """(g~ over S, mu over S, U, dg) of item (i, t) from the device's ua and the rebuilt null"""
    mu, Z, kappa = null
    Uv, a = r["ua"][i, t, 0], r["ua"][i, t, 2:]
    xt = x[i] + np.where(ms[i], xbar[i], 0.0)
    az = np.abs(Z * a[None, :]).sum(1)
    gt = np.where(s, xt - Z @ a, 0.0)
    dg = 8 * (Pc + 3) * kappa * EPS * float(az.max()) + (Pc + 3) * EPS * float((np.abs(xt) + az).max())
    return gt[s], mu[s], Uv, dg


def check_against_restatement(r, G, inc, nulls, firth_z, Pc, rows=None):
    """every item of the device's result r against firth_reference; returns (items, corrected)"""
    s = inc.astype(bool)
    x, ms, xbar = operand(G, inc, r["flipped"])
    K, T = r["z"].shape
    items = corrected = 0
    for t in range(T):
        for i in (range(K) if rows is None else rows):
            z = r["z"][i, t]
            got = tuple(r[k][i, t] for k in ("log10p", "firth_status", "firth_beta", "firth_se", "firth_lrt"))
            items += 1
            if z != z:
                assert got[1] == 0 and all(v != v for v in got[:1] + got[2:]), (i, t, got)
                continue
            normal = gpca.GpcaEngine.normal_log10p(z)
            if not (math.isfinite(z) and abs(z) >= firth_z):
                assert got[1] == 0 and all(v != v for v in got[2:]) and abs(got[0] - normal) <= 16 * EPS * max(normal, 1.0), (i, t, got, normal)
                continue
            g, mu, Uv, dg = item_inputs(r, x, ms, xbar, s, nulls[t], i, t, Pc)
            ref = firth_reference(g, mu, Uv, normal=normal)
            assert got[1] == 1 and ref["status"] == 1, (i, t, got, ref)
            corrected += 1
            sgn = -1.0 if r["flipped"][i] else 1.0
            bars = firth_bars(g, mu, Uv, ref, dg)
            for k, v, want in (("log10p", got[0], ref["log10p"]), ("beta", got[2], sgn * ref["beta"]), ("se", got[3], ref["se"]),
                               ("D", got[4], ref["D"])):
                d = abs(v - want)
                WORST[k] = max(WORST[k], d / bars[k])
                assert d <= bars[k], (i, t, k, v, want, bars[k])
            WORST["passes"] = max(WORST["passes"], ref["passes"])
    return items, corrected


# ------------------------------------------------------------------------------------------------ 1. the edge shapes
@pytest.mark.parametrize("N,T,Pc", CASES)
def test_firth_at_edge_shapes(N, T, Pc):
    G, Y, Cm, inc, special, nulls = inputs(N, T, Pc)
    res = {}
    for store in ("int8", "2bit"):
        with gpca.GpcaEngine(storage=STORES[store]) as e:
            load(e, G)
            res[store] = e.assoc_logistic_firth(Y, Cm, include=inc, max_vif=VIF, firth_z=0.0, ua=True)
    r = res["int8"]
    for k, v in r.items():                              # int8 and 2-bit residency: the same bits
        assert same(v, res["2bit"][k]), k
    assert all(r[k].shape == (M_ROWS, T) for k in ("log10p", "firth_status", "firth_beta", "firth_se", "firth_lrt"))
    items, corrected = check_against_restatement(r, G, inc, nulls, 0.0, Pc)
    st = r["firth_status"]
    print(f"N={N} T={T} Pc={Pc}: {items} items, status 0/1/2: {int((st == 0).sum())}/{int((st == 1).sum())}/{int((st == 2).sum())}, "
          f"NaN {int(np.isnan(r['z']).sum())}; worst / bar so far: " + ", ".join(f"{k} {v:.3g}" for k, v in WORST.items()))
    finite = np.isfinite(r["z"])
    assert items == M_ROWS * T and corrected == int(finite.sum()) and np.all(st[finite] == 1) and np.all(st[~finite] == 0)
    # the rows of the module docstring (trait 0)
    # (with 61 covariates the variance-inflation rule may refuse a singleton: the score scan's NaN, not this correction's)
    for row in (5, 6, 7):
        assert finite[row, 0] or Pc == 61, row
        if finite[row, 0]:
            assert np.isfinite(r["firth_beta"][row, 0]) and r["firth_se"][row, 0] > 0, row
    if finite[7, 0]:
        assert r["firth_beta"][7, 0] > 0 and r["firth_lrt"][7, 0] > 0                              # all carriers cases: finite, positive
    if special:
        assert np.all(np.isnan(r["log10p"][2])) and np.all(np.isnan(r["log10p"][M_ROWS // 2]))     # monomorphic; no observed call
        assert r["flipped"][0] == 1.0 and finite[0].all() and r["a1_freq"][0] > 0.5                 # the A1-frequent row is corrected


# ------------------------------------------------------------------------------------------------ 2. - 4. cutoffs, pass-through, bits
def test_cutoffs_passthrough_bands_and_storage_bits():
    N, T, Pc = 257, 2, 3
    G, Y, Cm, inc, _, nulls = inputs(N, T, Pc)
    out, at = {}, {}
    for name, store, prec in (("int8", _lib.STORE_INT8, _lib.PREC_I8_EXACT), ("2bit", _lib.STORE_2BIT, _lib.PREC_I8_EXACT),
                              ("f32", _lib.STORE_INT8, _lib.PREC_F32_MFMA)):
        with gpca.GpcaEngine(storage=store, precision=prec) as e:
            load(e, G)
            out[name] = e.assoc_logistic_firth(Y, Cm, include=inc, max_vif=VIF, ua=True)               # firth_z = 1.959964, the default
            if name != "int8":
                continue
            score = e.assoc_logistic_score(Y, Cm, include=inc, max_vif=VIF, ua=True)
            for fz in (0.0, float("inf")):
                at[fz] = e.assoc_logistic_firth(Y, Cm, include=inc, max_vif=VIF, firth_z=fz, ua=True)
            bands = [e.assoc_logistic_firth(Y, Cm, include=inc, max_vif=VIF, rows=b, ua=True) for b in BANDS]
    r = at[1.959964] = out["int8"]
    # pass-through: stats, ua and rowinfo carry the bits of gpca_assoc_logistic_score at every cutoff
    for fz, res in at.items():
        for k, v in score.items():
            assert same(v, res[k]), (fz, k)
    # firth_z = +inf: nothing is corrected, the value is the host's normal one
    off = at[float("inf")]
    assert np.all(off["firth_status"] == 0) and all(np.all(np.isnan(off[k])) for k in ("firth_beta", "firth_se", "firth_lrt"))
    items, corrected = check_against_restatement(off, G, inc, nulls, float("inf"), Pc)
    assert corrected == 0
    # the default cutoff: the items at or above it are corrected, held to the restatement; the others keep the normal value
    items, corrected = check_against_restatement(r, G, inc, nulls, 1.959964, Pc)
    flagged = np.abs(r["z"]) >= 1.959964
    assert 0 < corrected == int(flagged.sum()) < int(np.isfinite(r["z"]).sum())
    assert np.all(r["firth_status"][flagged] == 1) and np.all(r["firth_status"][~flagged] == 0)
    assert same(r["log10p"][~flagged], off["log10p"][~flagged])
    # an item corrected at both cutoffs has the same bits at both
    for k in ("log10p", "firth_beta", "firth_se", "firth_lrt"):
        assert same(r[k][flagged], at[0.0][k][flagged]), k
    # a band is the full call's rows, bit for bit; so are 2-bit residency and an f32-MFMA handle
    for (a, b), band in zip(BANDS, bands):
        for k, v in band.items():
            assert v.shape[0] == b - a and same(v, r[k][a:b]), (a, b, k)
    for name in ("2bit", "f32"):
        for k, v in out[name].items():
            assert same(v, r[k]), (name, k)


# ------------------------------------------------------------------------------------------------ 5. flip invariance
def test_flip_invariance():
    """Every row recoded as 2 - g (missing calls kept).  The operand is coded by the minor allele, so a row whose s1 differs from
    n_obs changes its flipped flag and keeps its operand: -log10 p, se and D keep their bits and beta^ (for A1) changes its sign, bit
    for bit.  Row 3 has s1 = n_obs (flipped in neither coding): its operand is recoded, g~ and U change sign, and the two runs start
    from two different f32 passes: their U and a_j differ by up to the sum of the two ua bars of tests/test_gpu_assoc_score.py
    (restate), so the bar is firth_bars with du = that sum and dg widened by max_n sum_j d a_j |Z_nj|, taken twice (once per run)."""
    N, T, Pc = 257, 2, 3
    G, Y, Cm, inc, special, nulls = inputs(N, T, Pc)
    assert special
    G2 = np.where(G == -127, G, 2 - G).astype(np.int8)
    Bs, kappas = panel(Y, Cm, inc, np.stack([n[0] for n in nulls], 1))
    uabar = restate(G, Bs, kappas, inc, Pc)["bar"] + restate(G2, Bs, kappas, inc, Pc)["bar"]
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        load(e, G)
        a = e.assoc_logistic_firth(Y, Cm, include=inc, max_vif=VIF, firth_z=0.0, ua=True)
        load(e, G2)
        b = e.assoc_logistic_firth(Y, Cm, include=inc, max_vif=VIF, firth_z=0.0, ua=True)
    tie = a["flipped"] == b["flipped"]
    live = ~np.isnan(a["z"][:, 0])
    assert tie[3] and live[3] and np.all(a["flipped"][~tie & live] + b["flipped"][~tie & live] == 1.0)
    for k in ("log10p", "firth_se", "firth_lrt", "firth_status"):
        assert same(a[k][~tie], b[k][~tie]), k
    assert same(a["firth_beta"][~tie], -b["firth_beta"][~tie]) and same(a["z"][~tie], -b["z"][~tie])
    s = inc.astype(bool)
    xa, msa, xbara = operand(G, inc, a["flipped"])
    seen = 0
    for t in range(T):
        for i in np.flatnonzero(tie & live):
            if not (np.isfinite(a["z"][i, t]) and np.isfinite(b["z"][i, t])):
                continue
            assert a["firth_status"][i, t] == 1 and b["firth_status"][i, t] == 1
            g, mu, Uv, dg = item_inputs(a, xa, msa, xbara, s, nulls[t], i, t, Pc)
            dg += float((np.abs(nulls[t][1]) @ uabar[i, t, 2:]).max())
            ref = firth_reference(g, mu, Uv, normal=0.0)
            bars = firth_bars(g, mu, Uv, ref, dg, du=float(uabar[i, t, 0]))
            for k, va, vb in (("log10p", a["log10p"][i, t], b["log10p"][i, t]), ("beta", a["firth_beta"][i, t], -b["firth_beta"][i, t]),
                              ("se", a["firth_se"][i, t], b["firth_se"][i, t]), ("D", a["firth_lrt"][i, t], b["firth_lrt"][i, t])):
                print(f"row {i} trait {t}: |d {k}| {abs(va - vb):.3g} of {2 * bars[k]:.3g}")
                assert abs(va - vb) <= 2 * bars[k], (i, t, k, va, vb)
            seen += 1
    assert seen >= T


# ------------------------------------------------------------------------------------------------ 6. across the 2^20-item list range
def test_across_the_list_range():
    """N = 63, T = 16, Pc = 1, 70 000 rows: 1 120 000 items, the second list range starts at item 2^20 = row 65 536.  firth_z = 3."""
    N, T, Pc, M = 63, 16, 1, 70000
    rng = np.random.default_rng(63016)
    p = rng.uniform(0.05, 0.5, M)[:, None]
    G = ((rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8))
    G[rng.random((M, N)) < 0.01] = -127
    Y = (rng.random((N, T)) < 0.3).astype(np.float64)
    Y[:3], Y[3:6] = 1.0, 0.0
    Cm = rng.standard_normal((N, Pc))
    inc = np.ones(N, np.uint8)
    nulls = rebuild(Y, Cm, inc)
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        load(e, G)
        r = e.assoc_logistic_firth(Y, Cm, include=inc, max_vif=VIF, firth_z=3.0, ua=True)
        score = e.assoc_logistic_score(Y, Cm, include=inc, max_vif=VIF, ua=True)
        band = e.assoc_logistic_firth(Y, Cm, include=inc, max_vif=VIF, firth_z=3.0, rows=(65000, 66000), ua=True)
    for k, v in score.items():
        assert same(v, r[k]), k
    for k, v in band.items():
        assert same(v, r[k][65000:66000]), k
    z, st = r["z"], r["firth_status"]
    flagged = np.isfinite(z) & (np.abs(z) >= 3.0)
    assert np.all(st[flagged] == 1) and np.all(st[~flagged] == 0)
    lo, hi = flagged[:65536], flagged[65536:]
    print(f"{int(flagged.sum())} of {flagged.size} items corrected: {int(lo.sum())} in the first range, {int(hi.sum())} in the second")
    assert lo.sum() > 100 and hi.sum() > 5
    # the flagged items of the rows around the boundary and of the last rows, against the restatement
    rows = sorted(set(np.flatnonzero(flagged[65000:66000].any(1))[:40] + 65000) | set(np.flatnonzero(flagged[69000:].any(1))[:10] + 69000))
    items, corrected = check_against_restatement(r, G, inc, nulls, 3.0, Pc, rows=rows)
    assert corrected >= 10


# ------------------------------------------------------------------------------------------------ 7. calibration through the device
def test_calibration_through_the_device():
    rows = calibration_rows()
    G = np.stack([x for x, _ in rows]).astype(np.int8)
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        load(e, G)
        for i, (x, yy) in enumerate(rows):
            r = e.assoc_logistic_firth(yy, None, rows=(i, i + 1))
            print(f"row {i}: z {r['z'][0, 0]:.2f}  device Firth {r['log10p'][0, 0]:.4f}  beta {r['firth_beta'][0, 0]:.3f}  se {r['firth_se'][0, 0]:.3f}")
            assert r["firth_status"][0, 0] == 1 and abs(r["log10p"][0, 0] - CALIBRATION[i]) <= 0.002


# ------------------------------------------------------------------------------------------------ 8. errors
def test_errors():
    N, T, Pc = 65, 1, 0
    G, Y, Cm, inc, _, _ = inputs(N, T, Pc)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    BA, ST = _lib.GPCA_ERR_BAD_ARG, _lib.GPCA_ERR_STATE
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        load(e, G)
        for bad in (-1e-300, -1.0, float("nan"), float("-inf")):
            with pytest.raises(GpcaError) as ei:
                e.assoc_logistic_firth(Y, None, include=inc, firth_z=bad)
            assert ei.value.status == BA and "firth_z" in ei.value.message
        for good in (0.0, 0.49, float("inf")):
            e.assoc_logistic_firth(Y, None, include=inc, firth_z=good)
        Yv, stats = np.ascontiguousarray(Y), np.zeros((M_ROWS, 1, 5))
        lib = _lib.load()
        assert lib.gpca_assoc_logistic_firth(e._h, vp(Yv), 1, None, 0, vp(inc), 50.0, 2.0, 0, M_ROWS, vp(stats), None, None, None) == BA   # NULL firth
        firth = np.zeros((M_ROWS, 1, 5))
        assert lib.gpca_assoc_logistic_firth(e._h, vp(Yv), 1, None, 0, vp(inc), 50.0, 2.0, 0, M_ROWS, None, vp(firth), None, None) == 0    # firth alone
        assert lib.gpca_assoc_logistic_firth(None, vp(Yv), 1, None, 0, vp(inc), 50.0, 2.0, 0, M_ROWS, None, vp(firth), None, None) == BA
        for kw in (dict(max_vif=0.5), dict(rows=(0, M_ROWS + 1))):                                  # the score call's refusals hold
            with pytest.raises(GpcaError) as ei:
                e.assoc_logistic_firth(Y, None, include=inc, **kw)
            assert ei.value.status == BA
        with pytest.raises(GpcaError) as ei:
            e.assoc_logistic_firth(np.ones((N, 1)), None, include=inc)                             # one class
        assert ei.value.status == BA
    with gpca.GpcaEngine() as e:                                                         # a streamed handle
        e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), M_ROWS, N, panel_rows=256, ring_slots=2, fused=False)
        e.snp_stats(gpca.QcConfig.none())
        with pytest.raises(GpcaError) as ei:
            e.assoc_logistic_firth(Y, None, include=inc)
        assert ei.value.status == ST and "gpca_assoc_logistic_firth" in ei.value.message and "panel" in ei.value.message
    with gpca.GpcaEngine() as e:                                                         # a hooked (row-sharded) handle
        e.upload_genotypes_i8(G[:20].copy())
        e.set_allreduce_hook(lambda buf: None, 2, 0, 0)
        e.set_standardization(np.ones(20, np.float32), np.ones(20, np.float32), np.ones(20, np.uint8))
        with pytest.raises(GpcaError) as ei:
            e.assoc_logistic_firth(Y, None, include=inc)
        assert ei.value.status == ST and "shard" in ei.value.message
