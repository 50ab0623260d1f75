"""CPU-only: the saddle-point correction of the logistic score scan on the host -- gpca_spa_log10p (include/gpca.h section a14; the
rules of csrc/spa_math.h that the kernel of assoc_spa.hip runs too), gpca_normal_log10p's bits, io.write_assoc_logistic with the SPA
column and its twin in host/formats.hpp, and the rules of --gpca-assoc-spa / --gpca-assoc-spa-z in both programs.

This module holds a numpy f64 restatement of section a14 (spa_reference): the same per-sample forms, the same guarded Newton, the same
tail, with numpy's pairwise sums.  It is the reference of tests/test_gpu_assoc_spa.py as well.

The bar (spa_bars), for an item with both implementations on the same side of every decision.  e = 2^-53; a sum of n terms in any
order is within (n + 4) e sum |term| of the exact sum of the rounded terms (n - 1 additions, and the terms themselves carry a few
roundings of exp / expm1 / log1p and the products: the "+ 4").  Write E0, E1, E2 for that bound on K, K' and K'' at the root.
 * zeta.  Both implementations stop when |tau' - tau| <= 1e-10 (1 + |tau|) and return tau'.  Newton converges quadratically here, so the
   returned tau' is closer to the root of the computed K' than the last step was long: each is within 1e-10 (1 + |zeta|) of its own
   root, and the two computed K' differ by at most 2 E1, which moves the root by 2 E1 / K''.  An input error dg in every g~_n (the GPU
   test's reconstruction of Z; 0 here) moves K' by at most dK1 = dg sum_n w_n (1 + |g~_n zeta|) (d/dg of a term of K' is w_n times
   a factor at most 1 + |a| in magnitude), hence
       bar_zeta = 2e-10 (1 + |zeta|) + (2 E1 + dK1) / K''(zeta).
 * A = zeta c - K(zeta).  dA / dzeta = c - K'(zeta) = 0 at the root, so an error d in zeta moves A only by K'' d^2 / 2 (the issue's
   remark); the sums add E0, the product zeta c one rounding, and dg moves K by at most dg sum_n w_n |zeta| (1 + |a_n|) =: dK0:
       dA = K'' bar_zeta^2 / 2 + 2 E0 + 2 e |zeta c| + dK0;        w = sign(zeta) sqrt(2 A):  dw = dA / |w| + 2 e |w|.
 * v = zeta sqrt(K'').  |K'''| <= max |g~| K'' (the derivative of a term of K'' is g~ times the term times a factor in [-1, 1]):
       dv = |v| (bar_zeta / |zeta| + (max |g~| bar_zeta + (2 E2 + dK2) / K'') / 2 + 2 e),   dK2 = dg sum_n w_n |g~_n| (2 + |a_n|).
 * r = w + log(v / w) / w:  dr = |1 - (1 + log(v / w)) / w^2| dw + dv / |v w| + 4 e (|w| + |log(v / w) / w|).
 * The tail -log10(1 - Phi(|r|)) has slope phi / (1 - Phi) / ln 10 <= (|r| + 1) / ln 10 (Mills' ratio), and the function itself is
   held to 3.3e-15 relative by tests/test_assoc_score_host.py:
       bar_tail = (|r| + 1) dr / ln 10 + 4e-15 (tail + 1).
   The two-sided value is a log-sum of the tails, which moves by no more than its larger input error: bar = max over the live tails,
   plus 4 e for the log1p.
All of this is first order; the bars are doubled for the second-order terms (bar_zeta^2 against bar_zeta is below 1e-9).  Largest
measured ratio to the bar on this module's cases: 1.1e-5 for zeta, 1.9e-5 for -log10 p: both sides walk the same
Newton path, so they differ by their sums' rounding only, while the bar is led by the stopping rule's 2e-10.

Calibration (a condition on the method, not on the arithmetic): N = 2000, 40 cases, an intercept-only null (mu = 0.02), four carrier
patterns; the exact two-sided p by enumerating the carriers with a binomial over the rest.  |-log10 p_SPA - exact| <= 0.25 while the
normal value is more than 3 decades off (the restatement gives 0.19, 0.13, 0.015, 0.005 against 12.1, 11.6, 7.9, 3.3)."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from genomic_pca_amd import _lib, io as gio
from genomic_pca_amd.cli import main
from genomic_pca_amd.engine import GpcaEngine
import genomic_pca_amd as gpca_pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "genomic_pca_amd", "bin", "genomic_pca")
EPS = 2.0 ** -53
LN10 = math.log(10.0)
INF = float("inf")


# ------------------------------------------------------------------------------------------------ the restatement of section a14
def normal_log10p_ref(z):
    """-log10(2 Phi(-|z|)), from math.erfc up to |z| = 37 and its asymptotic series beyond (relative error below 1e-15 there)"""
    z = abs(float(z))
    if z != z:
        return z
    if z == INF:
        return INF
    if z < 37.0:
        x = z / math.sqrt(2.0)
        return -math.log1p(-math.erf(x)) / LN10 if x < 0.5 else -math.log(math.erfc(x)) / LN10
    x2 = z * z / 2.0
    s, term = 1.0, 1.0
    for k in range(1, 12):
        term *= -(2 * k - 1) / (2.0 * x2)
        s += term
    return (x2 + 0.5 * math.log(math.pi * x2) - math.log(s)) / LN10


def k_terms(g, mu, tau):
    """the per-sample terms of K, K', K'' at tau in the forms that take only exp(-|a|)"""
    with np.errstate(all="ignore"):
        w = (1.0 - mu) * mu
        a = g * tau
        e, em = np.exp(-np.abs(a)), np.expm1(-np.abs(a))
        pos = a > 0
        D = np.where(pos, (1.0 - mu) * e + mu, (1.0 - mu) + mu * e)
        k1 = w * g * (np.where(pos, -em, em) / D)
        k2 = w * (g * g) * e / (D * D)
        k0 = np.where(pos, a * (1.0 - mu) + np.log1p((1.0 - mu) * np.expm1(-np.abs(a))), np.log1p(mu * np.expm1(-np.abs(a))) - a * mu)
        live = w > 0
        return np.where(live, k0, 0.0), np.where(live, k1, 0.0), np.where(live, k2, 0.0)


def spa_root_ref(g, mu, c):
    """(converged, zeta) by the guarded Newton of section a14"""
    sign = lambda x: int(x > 0) - int(x < 0)
    ev = lambda t: tuple(float(np.sum(x)) for x in k_terms(g, mu, t)[1:])
    tau, prev = 0.0, INF
    k1, k2 = ev(tau)
    k = k1 - c
    for _ in range(100):
        with np.errstate(all="ignore"):
            tn = float(np.float64(tau) - np.float64(k) / np.float64(k2))
        if not math.isfinite(tn):
            return False, tau
        if abs(tn - tau) <= 1e-10 * (1.0 + abs(tau)):
            return True, tn
        k1n, k2n = ev(tn)
        kn = k1n - c
        if sign(k) != sign(kn):
            if abs(tn - tau) > prev - 1e-10:
                tn = tau + sign(kn - k) * prev / 2.0
                k1n, k2n = ev(tn)
                kn = k1n - c
                prev = prev / 2.0
            else:
                prev = abs(tn - tau)
        tau, k, k2 = tn, kn, k2n
    return False, tau


def spa_reference(g, mu, u, normal=None):
    """Section a14 for one vector: a dict with log10p, status, zeta (2), and per tail what spa_bars needs"""
    g, mu = np.asarray(g, np.float64), np.asarray(mu, np.float64)
    w = (1.0 - mu) * mu
    p, q = g * (1.0 - mu), -g * mu
    hi, lo = float(np.sum(np.maximum(p, q))), float(np.sum(np.minimum(p, q)))
    V = float(np.sum(w * g * g))
    if normal is None:
        with np.errstate(all="ignore"):
            normal = 0.0 if u == 0 else normal_log10p_ref(float(np.float64(u) / np.sqrt(np.float64(V))))
    out = {"log10p": normal, "status": 0, "zeta": [math.nan, math.nan], "hi": hi, "lo": lo, "V": V, "tails": [None, None], "normal": normal}
    if u == 0 or u != u:
        return out
    s = abs(u)
    nl, ok = [INF, INF], True
    for side, c in ((0, s), (1, -s)):
        if (s >= hi) if side == 0 else (-s <= lo):
            out["zeta"][side] = INF if side == 0 else -INF
            continue
        conv, z = spa_root_ref(g, mu, c)
        out["zeta"][side] = z
        if not conv:
            ok = False
            continue
        t0, t1, t2 = k_terms(g, mu, z)
        K, K2 = float(np.sum(t0)), float(np.sum(t2))
        with np.errstate(all="ignore"):
            ww = np.sign(z) * np.sqrt(np.float64(2.0 * (z * c - K)))
            v = z * np.sqrt(np.float64(K2))
            r = float(ww + np.log(np.float64(v) / ww) / ww)
        tail = {"c": c, "zeta": z, "K": K, "K2": K2, "w": float(ww), "v": float(v), "r": r, "abs0": float(np.sum(np.abs(t0))),
                "abs1": float(np.sum(np.abs(t1))), "abs2": float(np.sum(np.abs(t2)))}
        out["tails"][side] = tail
        if not math.isfinite(r) or (r != 0 and (r > 0) != (c > 0)):
            ok = False
            continue
        nl[side] = normal_log10p_ref(r) + math.log10(2.0)
        tail["nlp"] = nl[side]
    if not ok:
        out["status"] = 2
        return out
    out["status"] = 1
    m, M = min(nl), max(nl)
    out["log10p"] = m if m == INF else m - math.log1p(10.0 ** (-(M - m))) / LN10
    return out


def spa_bars(g, mu, ref, dg=0.0, du=0.0):
    """(bar of zeta+ and zeta-, bar of -log10 p) for a status-1 item, as the module's docstring derives them; dg: an error bound of
    every entry of g; du: an error bound of U (it moves the target c: the root by du / K'', A = zeta c - K by |zeta| du)"""
    g, mu = np.asarray(g, np.float64), np.asarray(mu, np.float64)
    n, w = g.size, (1.0 - mu) * mu
    bz, bp = [0.0, 0.0], 4 * EPS
    for side, t in enumerate(ref["tails"]):
        if t is None:
            continue
        z, c = t["zeta"], t["c"]
        a = np.abs(g * z)
        E0, E1, E2 = ((n + 4) * EPS * t[k] for k in ("abs0", "abs1", "abs2"))
        dK1 = dg * float(np.sum(w * (1 + a)))
        dK0 = dg * float(np.sum(w * abs(z) * (1 + a)))
        dK2 = dg * float(np.sum(w * np.abs(g) * (2 + a)))
        bzeta = 2e-10 * (1 + abs(z)) + (2 * E1 + dK1 + du) / t["K2"]
        dA = t["K2"] * bzeta ** 2 / 2 + 2 * E0 + 2 * EPS * abs(z * c) + dK0 + abs(z) * du
        ww, v, r = abs(t["w"]), abs(t["v"]), t["r"]
        dw = dA / ww + 2 * EPS * ww
        dv = v * (bzeta / abs(z) + (float(np.max(np.abs(g))) * bzeta + (2 * E2 + dK2) / t["K2"]) / 2 + 2 * EPS)
        lg = math.log(v / ww)
        dr = abs(1 - (1 + lg) / ww ** 2) * dw + dv / (v * ww) + 4 * EPS * (ww + abs(lg / ww))
        bz[side] = 2 * bzeta
        bp = max(bp, 2 * ((abs(r) + 1) * dr / LN10 + 4e-15 * (t["nlp"] + 1)) + 4 * EPS)
    return bz, bp


def near_decision(g, mu, u, ref, dg=0.0):
    """True where the restatement itself stands within its summation error of the support rule's decision (s against a bound)"""
    g, mu = np.asarray(g, np.float64), np.asarray(mu, np.float64)
    bar = (g.size + 4) * EPS * max(ref["hi"], -ref["lo"]) + dg * g.size
    return abs(abs(u) - ref["hi"]) <= bar or abs(-abs(u) - ref["lo"]) <= bar


# ------------------------------------------------------------------------------------------------ 1. gpca_spa_log10p against it
def random_case(n, seed):
    rng = np.random.default_rng(1000 * n + seed)
    kind = seed % 3
    if kind == 0:                                       # a rare variant in an unbalanced trait, one covariate taken out
        mu = np.clip(0.03 * np.exp(0.8 * rng.standard_normal(n)), 1e-4, 0.5)
        x = (rng.random(n) < 0.02).astype(np.float64) * (1 + (rng.random(n) < 0.1))
        if not x.any():
            x[rng.integers(n)] = 1.0
    elif kind == 1:                                     # a common variant, balanced
        mu = rng.uniform(0.2, 0.8, n)
        x = rng.integers(0, 3, n).astype(np.float64)
        x[0], x[-1] = 0.0, 2.0                          # (never monomorphic)
    else:                                               # anything
        mu = rng.uniform(0.01, 0.99, n)
        x = rng.standard_normal(n)
    w = mu * (1 - mu)
    g = x - (w @ x) / w.sum() if n > 1 else x + 0.5
    V = float(np.sum(w * g * g))
    zt = (0.6, 2.0, 3.5, 6.0, 9.0)[seed % 5]
    p, q = g * (1 - mu), -g * mu
    hi, lo = float(np.sum(np.maximum(p, q))), float(np.sum(np.minimum(p, q)))
    u = zt * math.sqrt(V) * (1 if seed % 2 else -1)
    if seed % 7 != 3:                                   # mostly inside the support on the side of u; now and then beyond it
        u = math.copysign(min(abs(u), 0.9 * (hi if u > 0 else -lo)), u)
    return g, mu, u


@pytest.mark.parametrize("n", [1, 2, 63, 2049])
def test_spa_log10p_against_restatement(n):
    worst_z = worst_p = 0.0
    seen = set()
    for seed in range(30):
        g, mu, u = random_case(n, seed)
        ref = spa_reference(g, mu, u)
        lp, st, zeta = GpcaEngine.spa_log10p(g, mu, u)
        s = abs(u)
        margin = min(abs(s - ref["hi"]) / max(ref["hi"], 1e-300), abs(-s - ref["lo"]) / max(-ref["lo"], 1e-300))
        assert margin > 1e-9, (n, seed, "the case stands on a support decision")
        assert st == ref["status"], (n, seed, st, ref["status"], zeta, ref["zeta"])
        seen.add(st)
        for side in range(2):
            assert math.isinf(zeta[side]) == math.isinf(ref["zeta"][side]), (n, seed, side, zeta, ref["zeta"])
        if st != 1:
            assert lp == pytest.approx(ref["normal"], rel=1e-12)
            continue
        bz, bp = spa_bars(g, mu, ref)
        for side in range(2):
            if math.isinf(ref["zeta"][side]):
                assert zeta[side] == ref["zeta"][side]
                continue
            dz = abs(zeta[side] - ref["zeta"][side])
            worst_z = max(worst_z, dz / bz[side])
            assert dz <= bz[side], (n, seed, side, zeta, ref["zeta"], bz)
        if math.isinf(ref["log10p"]):
            assert lp == ref["log10p"]
            continue
        dp = abs(lp - ref["log10p"])
        worst_p = max(worst_p, dp / bp)
        assert dp <= bp, (n, seed, lp, ref["log10p"], bp)
    print(f"n={n}: statuses {sorted(seen)}; worst |d zeta| / bar {worst_z:.3g}, worst |d log10p| / bar {worst_p:.3g}")
    assert 1 in seen


# ------------------------------------------------------------------------------------------------ 2. calibration
def calibration_rows():
    """(genotype vector, y) of the four N = 2000, 40-case rows: carriers first, the cases among them first"""
    rows = []
    for het, hom, case_het, case_hom in ((6, 0, 3, 0), (7, 1, 2, 1), (20, 0, 5, 0), (40, 2, 6, 0)):
        N, cases = 2000, 40
        x = np.zeros(N)
        x[:het] = 1.0
        x[het:het + hom] = 2.0
        y = np.zeros(N)
        y[:case_het] = 1.0
        y[het:het + case_hom] = 1.0
        rest = cases - case_het - case_hom
        y[het + hom:het + hom + rest] = 1.0
        rows.append((x, y))
    return rows


def exact_log10p(x, y):
    """-log10 of the exact two-sided P(|U| >= |u_obs|), y_n independent Bernoulli(mu): the carriers' calls enumerated by how many of
    each dosage are cases (binomials), the non-carriers contribute -xbar (y - mu) each, a binomial count"""
    N, mu = x.size, float(y.mean())
    xbar = float(x.mean())
    g = x - xbar
    u_obs = float(g @ (y - mu))
    n1, n2 = int((x == 1).sum()), int((x == 2).sum())
    n0 = N - n1 - n2
    lg = math.lgamma
    pm = lambda n, k: math.exp(lg(n + 1) - lg(k + 1) - lg(n - k + 1) + k * math.log(mu) + (n - k) * math.log1p(-mu))
    p0 = np.array([pm(n0, k) for k in range(n0 + 1)])
    k0 = np.arange(n0 + 1)
    tot = 0.0
    base = -mu * float(g.sum())                          # (0 up to rounding: sum g = 0)
    for a in range(n1 + 1):
        for b in range(n2 + 1):
            uu = base + a * (1 - xbar) + b * (2 - xbar) + k0 * (0 - xbar)
            sel = np.abs(uu) >= abs(u_obs) * (1 - 1e-12)
            tot += pm(n1, a) * pm(n2, b) * float(p0[sel].sum())
    return -math.log10(tot), u_obs, g, mu


def test_calibration_against_exact_enumeration():
    want_spa, want_norm = (0.19, 0.13, 0.015, 0.005), (12.1, 11.6, 7.9, 3.3)
    for i, (x, y) in enumerate(calibration_rows()):
        exact, u, g, mu = exact_log10p(x, y)
        muv = np.full(x.size, mu)
        lp, st, zeta = GpcaEngine.spa_log10p(g, muv, u)
        z = u / math.sqrt(float(np.sum(mu * (1 - mu) * g * g)))
        norm = GpcaEngine.normal_log10p(z)
        ref = spa_reference(g, muv, u)
        print(f"row {i}: z {z:.2f}  exact {exact:.3f}  SPA {lp:.3f} (restatement {ref['log10p']:.3f}, status {st})  normal {norm:.2f}")
        assert st == 1 and abs(lp - exact) <= 0.25 and abs(norm - exact) > 3.0
        assert abs(abs(lp - exact) - want_spa[i]) <= 0.01 + 0.05 * want_spa[i] and abs(abs(norm - exact) - want_norm[i]) <= 0.06


# ------------------------------------------------------------------------------------------------ 3. - 5. the rules
def test_support_rule():
    """a target at or beyond a bound of the support: that tail is 0, its zeta +-inf, the status 1"""
    g, muv, u = np.array([1.0, -1.0]), np.array([0.1, 0.9]), 1.0                # the support is [-0.2, 1.8]
    ref = spa_reference(g, muv, u)
    assert -abs(u) <= ref["lo"] and abs(u) < ref["hi"]
    lp, st, zeta = GpcaEngine.spa_log10p(g, muv, u)
    assert st == 1 and zeta[1] == -INF and math.isfinite(zeta[0]) and zeta[0] > 0
    assert lp == pytest.approx(ref["tails"][0]["nlp"], abs=1e-9)                # the two-sided value is the upper tail alone
    lp2, st2, zeta2 = GpcaEngine.spa_log10p(-g, muv, -u)                        # mirrored: the upper tail is the one without
    assert st2 == 1 and zeta2[0] == INF and zeta2[1] == pytest.approx(-zeta[0], rel=1e-9) and lp2 == pytest.approx(lp, abs=1e-9)
    # beyond both bounds: p = 0
    g2, mu2 = np.array([1.0, -0.5, 0.25]), np.array([0.3, 0.6, 0.5])
    hi = float(np.sum(np.maximum(g2 * (1 - mu2), -g2 * mu2)))
    for u2 in (hi, 2 * hi, -2 * hi):
        lp, st, zeta = GpcaEngine.spa_log10p(g2, mu2, u2)
        assert st == 1 and lp == INF and zeta == (INF, -INF), (u2, lp, st, zeta)
    # one sample: the support is two points
    lp, st, zeta = GpcaEngine.spa_log10p([2.0], [0.25], 1.0)
    assert st == 1 and zeta[1] == -INF and math.isfinite(zeta[0]) and math.isfinite(lp)


def test_overflow_and_zero_score():
    rng = np.random.default_rng(3)
    n = 200
    mu = rng.uniform(0.05, 0.95, n)
    g = 1e4 * rng.standard_normal(n)                                            # |g~ tau| passes 710 long before a root
    hi = float(np.sum(np.maximum(g * (1 - mu), -g * mu)))
    for u in (0.999999 * hi, -0.5 * hi, 1e3):
        lp, st, zeta = GpcaEngine.spa_log10p(g, mu, u)
        ref = spa_reference(g, mu, u)
        assert lp == lp and zeta[0] == zeta[0] and zeta[1] == zeta[1] and st == ref["status"], (u, lp, st, zeta, ref["status"])
    # the terms themselves at |a| far past 710, either sign
    for tau in (1e300, -1e300, 800.0, -800.0):
        t0, t1, t2 = k_terms(np.array([1.0, -1.0, 3.0]), np.array([0.3, 0.3, 1e-13]), tau)
        assert np.all(np.isfinite(t1)) and np.all(np.isfinite(t2)) and not np.any(np.isnan(t0))
    g1 = np.array([1.0, -1.0, 2.0])
    m1 = np.array([0.3, 0.3, 0.9])
    for u in (1.5999999, -1.19999):                                             # roots at |tau| of the order 10: a = g tau stays small; and
        lp, st, zeta = GpcaEngine.spa_log10p(g1 * 1e3, m1, u * 1e3)            # ... the same scaled: tau shrinks, a does not
        assert lp == lp and st in (1, 2)
    lp, st, zeta = GpcaEngine.spa_log10p(g, mu, 0.0)
    assert lp == 0.0 and st == 0 and zeta[0] != zeta[0] and zeta[1] != zeta[1]  # U = 0: p = 1
    lp, st, zeta = GpcaEngine.spa_log10p(np.zeros(5), np.full(5, 0.5), 0.0)
    assert lp == 0.0 and st == 0


def test_non_convergence_gives_the_normal_value():
    """a tail that fails (the root underflows: w = 0, r is not finite) and a root rule that does not converge (the target one ulp
    inside the bound, where the computed K' saturates below it and K'' underflows to 0): status 2 and the normal value"""
    rng = np.random.default_rng(8)
    mu = rng.uniform(0.2, 0.8, 50)
    g = rng.standard_normal(50)
    V = float(np.sum(mu * (1 - mu) * g * g))
    lp, st, zeta = GpcaEngine.spa_log10p(g, mu, 1e-200)
    ref = spa_reference(g, mu, 1e-200)
    assert ref["status"] == 2 and st == 2 and lp == pytest.approx(GpcaEngine.normal_log10p(1e-200 / math.sqrt(V)), rel=1e-12)
    found = 0
    for m in (0.3, 0.35, 0.6, 0.7, 0.15, 0.45, 0.55, 0.85):
        gg, mm = np.array([1.0]), np.array([m])
        hi = float(gg[0] * (1 - m))
        u = math.nextafter(hi, 0.0)
        ref = spa_reference(gg, mm, u)
        lp, st, zeta = GpcaEngine.spa_log10p(gg, mm, u)
        assert st == ref["status"], (m, st, ref["status"])
        if st == 2:
            found += 1
            assert lp == GpcaEngine.normal_log10p(u / math.sqrt(m * (1 - m))) and math.isfinite(zeta[0])
    print("targets one ulp inside the bound that do not converge:", found)
    assert found >= 1


# ------------------------------------------------------------------------------------------------ 6. gpca_normal_log10p keeps its bits
def test_normal_log10p_bits_unchanged():
    f = _lib.load().gpca_normal_log10p
    rows = [ln.split() for ln in open(os.path.join(ROOT, "tests", "golden", "normal_log10p_grid.txt")) if not ln.startswith("#")]
    assert len(rows) > 200
    for zh, vh in rows:
        z = struct.unpack("<d", struct.pack("<Q", int(zh, 16)))[0]
        for s in (z, -z):
            got = struct.unpack("<Q", struct.pack("<d", f(s)))[0]
            assert got == int(vh, 16), (z, f(s))


# ------------------------------------------------------------------------------------------------ the ABI's argument rules
def test_spa_log10p_argument_rules():
    lib = _lib.load()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    g, mu = np.array([1.0, -1.0]), np.array([0.5, 0.5])
    lp, st, z = C.c_double(0), C.c_int32(0), np.zeros(2)
    BA = _lib.GPCA_ERR_BAD_ARG
    assert lib.gpca_spa_log10p(vp(g), vp(mu), 2, 0.25, C.byref(lp), None, None) == 0 and lp.value > 0      # zeta, status may be NULL
    assert lib.gpca_spa_log10p(None, vp(mu), 2, 0.25, C.byref(lp), vp(z), C.byref(st)) == BA
    assert lib.gpca_spa_log10p(vp(g), None, 2, 0.25, C.byref(lp), vp(z), C.byref(st)) == BA
    assert lib.gpca_spa_log10p(vp(g), vp(mu), 0, 0.25, C.byref(lp), vp(z), C.byref(st)) == BA
    assert lib.gpca_spa_log10p(vp(g), vp(mu), 2, 0.25, None, vp(z), C.byref(st)) == BA
    for bad_u in (math.nan, INF):
        assert lib.gpca_spa_log10p(vp(g), vp(mu), 2, bad_u, C.byref(lp), vp(z), C.byref(st)) == BA
    for bad_mu in (-0.1, 1.1, math.nan):
        assert lib.gpca_spa_log10p(vp(g), vp(np.array([0.5, bad_mu])), 2, 0.25, C.byref(lp), vp(z), C.byref(st)) == BA
    assert lib.gpca_spa_log10p(vp(np.array([1.0, math.inf])), vp(mu), 2, 0.25, C.byref(lp), vp(z), C.byref(st)) == BA
    with pytest.raises(_lib.GpcaError):
        gpca_pkg.spa_log10p(g, np.array([0.5, 2.0]), 0.25)
    # mu = 0 or 1: the sample adds nothing
    a = gpca_pkg.spa_log10p([1.0, -1.0, 5.0, -7.0], [0.5, 0.5, 0.0, 1.0], 0.25)
    assert a == gpca_pkg.spa_log10p(g, mu, 0.25)


# ------------------------------------------------------------------------------------------------ the writer and its twin
def test_write_assoc_logistic_with_spa_against_a_literal_file(tmp_path):
    prefix = str(tmp_path / "out" / "run")
    nan = float("nan")
    args = (["1", "1", "X", "2"], [100, 2500000, 7, 9], ["rs1", "rs2", "rs3", "rs4"], ["A", "G", "T", "C"], [500.0, 499.0, 0.0, 12.0],
            [0.25, 0.123456789, nan, 0.5], [1.5, -2.5e-7, nan, 1e10], [0.5, 1e-7, nan, 123456789.0], [3.0, -2.5, nan, 0.0],
            [2.56789012, 1234.5678, nan, 0.0])
    path = gio.write_assoc_logistic(prefix, "cad", *args, spa=[1, 2, 0, 0])
    want = ("#CHROM\tPOS\tID\tA1\tOBS_CT\tA1_FREQ\tBETA\tSE\tZ_STAT\tLOG10P\tSPA\n"
            "1\t100\trs1\tA\t500\t0.25\t1.5\t0.5\t3\t2.56789\tY\n"
            "1\t2500000\trs2\tG\t499\t0.123457\t-2.5e-07\t1e-07\t-2.5\t1234.57\tF\n"
            "X\t7\trs3\tT\t0\tNA\tNA\tNA\tNA\tNA\tNA\n"
            "2\t9\trs4\tC\t12\t0.5\t1e+10\t1.23457e+08\t0\t0\tN\n")
    assert open(path).read() == want
    plain = gio.write_assoc_logistic(str(tmp_path / "plain" / "run"), "cad", *args)
    assert open(plain).read() == "\n".join(ln.rsplit("\t", 1)[0] for ln in want.split("\n")[:-1]) + "\n"
    with pytest.raises(ValueError):
        gio.write_assoc_logistic(prefix, "cad", *args, spa=[1, 2])
    exe = str(tmp_path / "dump_assoc_spa")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "genomic_pca_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp", "dump_assoc_spa.cpp"), "-lz", "-o", exe])
    pre_c = str(tmp_path / "c" / "run")
    out = subprocess.run([exe, pre_c], capture_output=True, text=True, check=True).stdout.split()
    assert open(pre_c + ".cad.assoc.logistic", "rb").read() == want.encode()
    assert out == ["%d" % gio.spa_z_ok(v) for v in (0.5, 2.0, INF, 0.49, 0.0, -1.0, math.nan, -INF)] == list("11100000")


# ------------------------------------------------------------------------------------------------ 7. the spa_z rule and the flags
BASE = ["--bed-file", "t.bed", "--ld-block-file", "l.txt", "--out", "x"]


def bad_flags(ph):
    E = ["--eigensnp", "--gpca-assoc-pheno", ph]
    return [
        (E + ["--gpca-assoc-spa"], "--gpca-assoc-spa needs --gpca-assoc-logistic"),
        (E + ["--gpca-assoc-spa-z", "3"], "--gpca-assoc-spa-z needs --gpca-assoc-spa"),
        (E + ["--gpca-assoc-logistic", "--gpca-assoc-spa-z", "3"], "--gpca-assoc-spa-z needs --gpca-assoc-spa"),
        (E + ["--gpca-assoc-logistic", "--gpca-assoc-spa", "--gpca-assoc-spa-z", "0.49"], "--gpca-assoc-spa-z must be at least 0.5, or inf"),
        (E + ["--gpca-assoc-logistic", "--gpca-assoc-spa", "--gpca-assoc-spa-z", "-1"], "--gpca-assoc-spa-z must be at least 0.5, or inf"),
        (E + ["--gpca-assoc-logistic", "--gpca-assoc-spa", "--gpca-assoc-spa-z", "nan"], "--gpca-assoc-spa-z must be at least 0.5, or inf"),
    ]


def test_spa_flags_in_both_programs(tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "genomic_pca_amd", "host"), "-s"])
    ph = str(tmp_path / "cc.pheno")
    with open(ph, "w") as f:
        f.write("FID IID cc\n" + "".join(f"f{i} s{i} {1 + i % 2}\n" for i in range(6)))
    for flags, msg in bad_flags(ph):
        with pytest.raises(SystemExit) as ei:
            main(BASE + flags)
        assert str(ei.value).startswith("error: ") and msg in str(ei.value), (flags, str(ei.value))
        r = subprocess.run([BIN, *BASE, *flags], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stderr == str(ei.value) + "\n", (flags, r.stderr)
    # accepted values get as far as the missing fileset
    for ok in ([], ["--gpca-assoc-spa-z", "0.5"], ["--gpca-assoc-spa-z", "inf"], ["--gpca-assoc-spa-z", "2.5"]):
        with pytest.raises(FileNotFoundError):
            main(BASE + ["--eigensnp", "--gpca-assoc-pheno", ph, "--gpca-assoc-logistic", "--gpca-assoc-spa"] + ok)
    helptext = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--gpca-assoc-spa" in helptext and "--gpca-assoc-spa-z" in helptext
    for v, want in ((0.5, True), (2.0, True), (INF, True), (0.49, False), (0.0, False), (-1.0, False), (math.nan, False), (-INF, False)):
        assert gio.spa_z_ok(v) is want
