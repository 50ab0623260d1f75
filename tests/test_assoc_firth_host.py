"""CPU-only: the approximate Firth correction of the logistic score scan on the host -- gpca_firth_log10p (include/gpca.h section a15; the
rules of csrc/spa_math.h that the kernel of assoc_firth.hip runs too).

This module holds a numpy f64 restatement of section a15 (firth_reference): the per-sample forms of tests/test_assoc_spa_host.py
(k_terms) with the third and fourth derivative's terms beside them, the same root rule, numpy's pairwise sums.  It is the reference of
tests/test_gpu_assoc_firth.py as well.

The bars (firth_bars), for an item on which both implementations reach the same stationary point.  e = 2^-53; a sum of n terms in any
order is within E_k = (n + 4) e sum |term| of the exact sum of the rounded terms (the bound of the saddle-point test), k = 0 .. 4 for
K .. K''''.  All sums are taken at beta^.
 * beta^.  Both implementations stop when the step delta = -u / d of the sums in hand is at most 1e-10 (1 + |beta|) long and return
   beta.  Newton converges quadratically here, so beta is within that step of the root of its own computed u: 2e-10 (1 + |beta^|) for
   the pair.  The two computed u = U - K' + K''' / (2 K'') differ by at most 2 Eu, Eu = E1 + E3 / (2 K'') + |K'''| E2 / (2 K''^2),
   which moves the root by 2 Eu / |d|.  An input error dg in every g~_n moves a term of K' by at most dg w (1 + |a|), of K''' by at
   most dg w g^2 (3 + |a|) (|1 - 2p| <= 1 and d/da of w (1 - 2p) is w (1 - 6w), at most w), of K'' by dg w |g| (2 + |a|); du is an
   error bound of U:
       bar_beta = 2e-10 (1 + |beta^|) + (2 Eu + dKu + du) / |d|,    dKu = dK1 + dK3 / (2 K'') + |K'''| dK2 / (2 K''^2).
 * D = 2 f, f = beta U - K + log(K'' / K''(0)) / 2.  df / dbeta = u, and |u(beta^)| <= |d| 1e-10 (1 + |beta^|) by the stopping rule,
   so an error b in beta moves f by at most |d| (b^2 / 2 + 1e-10 (1 + |beta^|) b).  The sums add E0 and (E2 / K'' + E2(0) / K''(0)) / 2
   each side, the product beta U and the logarithm a rounding each, dg moves K by dK0 = dg sum w |beta| (1 + |a|) and the log by
   (dK2 / K'' + dK2(0) / K''(0)) / 2:
       bar_D = 2 [|d| (b^2 / 2 + 1e-10 (1 + |beta^|) b) + 2 E0 + E2 / K'' + E2(0) / K''(0) + 4 e (|beta^ U| + |log| + |f|)
                  + dK0 + dKlog + |beta^| du],   b = bar_beta.
 * sqrt(D): |sqrt(a) - sqrt(b)| <= |a - b| / sqrt(max(a, b)) and <= sqrt(|a - b|); the smaller of the two is taken, which handles D
   near 0.  -log10 p = -log10(2 Phi(-r)), r = sqrt(D), has slope at most (r + 1) / ln 10 (Mills' ratio), and gpca_normal_log10p is
   held to 3.3e-15 relative by tests/test_assoc_score_host.py:
       bar_p = (r + 1) min(bar_D / r, sqrt(bar_D)) / ln 10 + 4e-15 (value + 1).
 * se = K''^(-1/2): bar_se = se [(|K'''| b + 2 E2 + dK2) / (2 K'') + 2 e].
All of this is first order; every bar is doubled.  Largest measured ratio to the bar on this module's cases: 2.6e-5 for beta^, 0.040
for -log10 p, 7.6e-4 for se, 0.23 for D: both sides walk the same path, so beta^ differs by the sums' rounding
while its bar is led by the stopping rule's 2e-10; D's bar is led by the rounding of K and of the logarithm, which is what D's
difference is made of (the largest ratios are at n = 1 and 2, where the n + 4 of the bound is smallest).

The answer is the stationary point the rule reaches from 0 (on tiny samples u can have more than one root), so the independent
checks, in np.longdouble, are |u(beta^)| <= |d(beta^)| 2e-10 (1 + |beta^|) + 2 Eu and f(beta^) >= -(the rounding of f), not a
bracketing solver's root.

|g~ beta| > 710 cannot be reached through the rule itself: a step is clamped to 5 / gmax and there are at most 50, so |g~ beta| stays
below 250.  The per-sample terms are therefore checked directly at |a| far past 710 (finite, both signs), and the rule with an
outlying g~ whose |a| runs to the clamp's limit.

Calibration (a condition on the method, not on the arithmetic): the four N = 2000, 40-case rows of tests/test_assoc_spa_host.py.
The restatement's Firth -log10 p is 4.629, 4.495, 5.050, 3.707 against the exact 4.248, 4.208, 4.940, 3.693 (SPA 4.439, 4.341,
4.956, 3.689; normal 16.39, 15.77, 12.81, 7.01): Firth's chi^2_1 value is within 0.4 of the exact one where the normal value is more
than 3 decades off; beta^ = 3.91, 3.12, 2.89, 1.88 with se 0.82, 0.74, 0.51, 0.42, at 6 to 7 passes."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from genomic_pca_amd import _lib
from genomic_pca_amd.engine import GpcaEngine
import genomic_pca_amd as gpca_pkg

from test_assoc_spa_host import EPS, LN10, INF, calibration_rows, exact_log10p, k_terms, normal_log10p_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {"beta": 0.0, "log10p": 0.0, "se": 0.0, "D": 0.0}


# ------------------------------------------------------------------------------------------------ the restatement of section a15
def firth_terms(g, mu, beta):
    """the per-sample terms of K .. K'''' at beta (f64: k_terms' forms; the tilted probability p and w = p (1 - p) beside them)"""
    t0, t1, t2 = k_terms(g, mu, beta)
    with np.errstate(all="ignore"):
        w0 = (1.0 - mu) * mu
        a = g * beta
        e = np.exp(-np.abs(a))
        pos = a > 0
        D = np.where(pos, (1.0 - mu) * e + mu, (1.0 - mu) + mu * e)
        p = np.where(pos, mu, mu * e) / D
        wt = w0 * e / (D * D)
        g2 = g * g
        t3 = g2 * g * wt * (1.0 - 2.0 * p)
        t4 = g2 * g2 * wt * (1.0 - 6.0 * wt)
        live = w0 > 0
    return t0, t1, t2, np.where(live, t3, 0.0), np.where(live, t4, 0.0)


def firth_reference(g, mu, u, normal=None):
    """Section a15 for one vector: a dict with log10p, status, beta, se, D, the passes, and the sums at beta with their sums of
    absolute terms (what firth_bars needs)"""
    g, mu = np.asarray(g, np.float64), np.asarray(mu, np.float64)
    sums = lambda b: tuple(float(np.sum(t)) for t in firth_terms(g, mu, b))
    gmax = float(np.max(np.abs(g)))
    if normal is None:
        with np.errstate(all="ignore"):
            V = np.float64(np.sum((1.0 - mu) * mu * g * g))
            normal = 0.0 if u == 0 else normal_log10p_ref(float(np.float64(u) / np.sqrt(V)))
    beta, f, ok, passes = 0.0, 0.0, False, 1
    P = sums(0.0)
    K20 = P[2]
    if K20 > 0 and math.isfinite(K20):
        for _ in range(50):
            k0, k1, k2, k3, k4 = (np.float64(v) for v in P)
            with np.errstate(all="ignore"):
                us = np.float64(u) - k1 + k3 / (2.0 * k2)
                d = -k2 + (k4 * k2 - k3 * k3) / (2.0 * (k2 * k2))
                delta = float(-us / d if d < 0 else us / k2)
            if not math.isfinite(delta):
                break
            if abs(delta) <= 1e-10 * (1.0 + abs(beta)):
                ok = True
                break
            if abs(delta) * gmax > 5.0:
                delta = math.copysign(5.0, delta) / gmax
            small = abs(delta) <= 1e-4 * (1.0 + abs(beta))
            got = False
            for h in range(11):
                bt = beta + delta * 2.0 ** -h
                Pt = sums(bt)
                passes += 1
                with np.errstate(all="ignore"):
                    ft = float(np.float64(bt) * np.float64(u) - np.float64(Pt[0]) + 0.5 * np.log(np.float64(Pt[2]) / np.float64(K20)))
                if math.isfinite(ft) and Pt[2] > 0 and (small or ft >= f):
                    got = True
                    break
            if not got:
                break
            beta, P, f = bt, Pt, ft
    D = max(2.0 * f, 0.0) if f == f else 0.0
    with np.errstate(all="ignore"):
        se = float(1.0 / np.sqrt(np.float64(P[2])))
    t = firth_terms(g, mu, beta)
    return {"log10p": normal_log10p_ref(math.sqrt(D)) if ok else normal, "status": 1 if ok else 2, "beta": beta, "se": se, "D": D, "f": f,
            "passes": passes, "normal": normal, "K": P, "K20": K20, "abs": tuple(float(np.sum(np.abs(x))) for x in t),
            "abs20": float(np.sum(np.abs(firth_terms(g, mu, 0.0)[2])))}


def firth_ud(ref, u):
    k0, k1, k2, k3, k4 = ref["K"]
    return u - k1 + k3 / (2 * k2), -k2 + (k4 * k2 - k3 * k3) / (2 * k2 * k2)


def firth_bars(g, mu, u, ref, dg=0.0, du=0.0):
    """the doubled bars of beta, -log10 p, se and D for a status-1 item, as the module's docstring derives them"""
    g, mu = np.asarray(g, np.float64), np.asarray(mu, np.float64)
    n, b = g.size, ref["beta"]
    k0, k1, k2, k3, k4 = ref["K"]
    E = [(n + 4) * EPS * a for a in ref["abs"]]
    E20 = (n + 4) * EPS * ref["abs20"]
    _, d = firth_ud(ref, u)
    a = np.abs(g * b)
    w = firth_terms(g, mu, b)[2]
    with np.errstate(all="ignore"):
        w = np.where(g != 0, w / (g * g), 0.0)                # the tilted w = p (1 - p) of every sample
    w0 = (1 - mu) * mu
    ag = np.abs(g)
    dK1, dK2, dK3 = dg * float(np.sum(w * (1 + a))), dg * float(np.sum(w * ag * (2 + a))), dg * float(np.sum(w * ag * ag * (3 + a)))
    dK0 = dg * float(np.sum(w * abs(b) * (1 + a)))
    dK20 = dg * float(np.sum(w0 * ag * 2))
    Eu = E[1] + E[3] / (2 * k2) + abs(k3) * E[2] / (2 * k2 * k2)
    dKu = dK1 + dK3 / (2 * k2) + abs(k3) * dK2 / (2 * k2 * k2)
    stop = 1e-10 * (1 + abs(b))
    bb = 2 * stop + (2 * Eu + dKu + du) / abs(d)
    lg = abs(math.log(k2 / ref["K20"]))
    bD = 2 * (abs(d) * (bb * bb / 2 + stop * bb) + 2 * E[0] + E[2] / k2 + E20 / ref["K20"] + 4 * EPS * (abs(b * u) + lg + abs(ref["f"]))
              + dK0 + (dK2 / k2 + dK20 / ref["K20"]) / 2 + abs(b) * du)
    r = math.sqrt(ref["D"])
    ds = min(bD / r, math.sqrt(bD)) if r > 0 else math.sqrt(bD)
    bp = (r + 1) * ds / LN10 + 4e-15 * (ref["log10p"] + 1)
    bse = ref["se"] * ((abs(k3) * bb + 2 * E[2] + dK2) / (2 * k2) + 2 * EPS)
    return {"beta": 2 * bb, "log10p": 2 * bp, "se": 2 * bse, "D": 2 * bD, "Eu": Eu + dKu + du, "stop": stop}


def check_item(got, g, mu, u, ref, dg=0.0, du=0.0, worst=WORST, tag=None):
    """got = (log10p, status, beta, se, D) of an implementation against the restatement's ref, status 1 on both sides"""
    bars = firth_bars(g, mu, u, ref, dg, du)
    for k, v in (("log10p", got[0]), ("beta", got[2]), ("se", got[3]), ("D", got[4])):
        dlt = abs(v - ref[k])
        worst[k] = max(worst[k], dlt / bars[k])
        assert dlt <= bars[k], (tag, k, v, ref[k], bars[k])
    return bars


def independent_checks(g, mu, u, beta, bars):
    """np.longdouble: |u(beta^)| <= |d| 2e-10 (1 + |beta^|) + 2 Eu and f(beta^) >= -(its rounding); returns f"""
    L = np.longdouble
    g, mu, b = np.asarray(g, L), np.asarray(mu, L), L(beta)
    live = (1 - mu) * mu > 0
    g, mu = g[live], mu[live]
    a = g * b
    with np.errstate(all="ignore"):
        # in the forms that take only exp(-|a|), in extended precision
        e = np.exp(-np.abs(a))
        Dn = np.where(a > 0, (1 - mu) * e + mu, (1 - mu) + mu * e)
        p = np.where(a > 0, mu, mu * e) / Dn
        K = np.sum(np.where(a > 0, a * (1 - mu) + np.log1p((1 - mu) * np.expm1(-np.abs(a))), np.log1p(mu * np.expm1(-np.abs(a))) - a * mu))
    w = p * (1 - p)
    K1, K2, K3, K4 = np.sum(g * (p - mu)), np.sum(g * g * w), np.sum(g ** 3 * w * (1 - 2 * p)), np.sum(g ** 4 * w * (1 - 6 * w))
    K20 = np.sum(g * g * mu * (1 - mu))
    us = L(u) - K1 + K3 / (2 * K2)
    d = -K2 + (K4 * K2 - K3 * K3) / (2 * K2 * K2)
    assert abs(float(us)) <= abs(float(d)) * 2 * bars["stop"] + 2 * bars["Eu"], (float(us), float(d), bars)
    f = float(b * L(u) - K + np.log(K2 / K20) / 2)
    assert f >= -bars["D"], (f, bars["D"])
    return f


# ------------------------------------------------------------------------------------------------ 1. gpca_firth_log10p against it
KINDS = ("all cases", "all controls", "one carrier", "U = 0", "balanced common", "anything")


def make_case(n, kind, seed):
    """(g~, mu, u, y): an intercept-adjusted vector and the score it has for a drawn y"""
    rng = np.random.default_rng(7000 * n + 10 * seed + KINDS.index(kind))
    rare = kind in KINDS[:3]
    if rare:
        mu = np.clip(0.05 * np.exp(0.8 * rng.standard_normal(n)), 1e-3, 0.5)
        x = np.zeros(n)
        ncar = 1 if kind == "one carrier" else max(1, n // 40)
        car = rng.choice(n, size=min(ncar, n), replace=False)
        x[car] = 1.0 + (rng.random(car.size) < 0.15)
    elif kind == "anything":
        mu = rng.uniform(0.01, 0.99, n)
        x = rng.standard_normal(n)
    else:
        mu = rng.uniform(0.2, 0.8, n)
        x = rng.integers(0, 3, n).astype(np.float64)
        x[0], x[-1] = 0.0, 2.0
    w = mu * (1 - mu)
    g = x - (w @ x) / w.sum() if n > 1 else x + 0.5
    y = (rng.random(n) < mu).astype(np.float64)
    if kind == "all cases":
        y[x > 0] = 1.0
    elif kind == "all controls":
        y[x > 0] = 0.0
    elif kind == "one carrier":
        y[x > 0] = float(seed % 2)
    u = 0.0 if kind == "U = 0" else float(g @ (y - mu))
    return g, mu, u, y


@pytest.mark.parametrize("n", [1, 2, 63, 2049])
def test_firth_log10p_against_restatement(n):
    worst = dict.fromkeys(WORST, 0.0)
    most = 0
    for kind in KINDS:
        for seed in range(5):
            g, mu, u, y = make_case(n, kind, seed)
            ref = firth_reference(g, mu, u)
            got = GpcaEngine.firth_log10p(g, mu, u)
            tag = (n, kind, seed)
            assert ref["status"] == 1 and got[1] == 1, (tag, got, ref)          # separation included: finite, corrected
            assert all(math.isfinite(v) for v in got), (tag, got)
            bars = check_item(got, g, mu, u, ref, worst=worst, tag=tag)
            f = independent_checks(g, mu, u, got[2], bars)
            assert abs(max(2 * f, 0.0) - got[4]) <= bars["D"], (tag, f, got[4])
            most = max(most, ref["passes"])
            if kind == "all cases" and n >= 63:
                assert got[2] > 0 and got[4] > 0
            if kind == "all controls" and n == 2049:                            # (51 carriers; one control carrier alone says little)
                assert got[2] < 0
    for k in WORST:
        WORST[k] = max(WORST[k], worst[k])
    print(f"n={n}: most passes {most}; worst / bar: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_separation_is_finite_where_the_score_beta_is_not():
    """six carriers, all of them cases, in 2000 samples with 40 cases: the maximum-likelihood beta is +inf; Firth's is finite"""
    x, y = np.zeros(2000), np.zeros(2000)
    x[:6] = 1.0
    y[:40] = 1.0
    mu = np.full(2000, 0.02)
    g = x - x.mean()
    u = float(g @ (y - mu))
    lp, st, beta, se, D = GpcaEngine.firth_log10p(g, mu, u)
    ref = firth_reference(g, mu, u)
    assert st == 1 and 3.0 < beta < 12.0 and 0.0 < se < 5.0 and ref["passes"] <= 12, (lp, beta, se, D, ref["passes"])
    check_item((lp, st, beta, se, D), g, mu, u, ref)
    # the unpenalised score keeps growing: U - K'(b) > 0 at every b (no finite maximum)
    for b in (1.0, 10.0, 30.0):
        assert u - float(np.sum(k_terms(g, mu, b)[1])) > 0


def test_terms_past_710_and_an_outlier():
    for beta in (1e300, -1e300, 800.0, -800.0):
        t = firth_terms(np.array([1.0, -1.0, 3.0]), np.array([0.3, 0.3, 1e-13]), beta)
        assert all(np.all(np.isfinite(x)) for x in t[1:]) and not np.any(np.isnan(t[0]))
    # the library's terms at the same arguments, through a one-sample call: the pass at 0 and the first clamped step are finite
    rng = np.random.default_rng(5)
    n = 300
    mu = rng.uniform(0.05, 0.95, n)
    g = rng.standard_normal(n)
    g[0] = 4e3                                                                  # gmax: every step is clamped to 5 / 4e3
    y = (rng.random(n) < mu).astype(np.float64)
    u = float(g @ (y - mu))
    got = GpcaEngine.firth_log10p(g, mu, u)
    ref = firth_reference(g, mu, u)
    assert got[1] == ref["status"] and all(v == v for v in got), (got, ref)
    if got[1] == 1:
        check_item(got, g, mu, u, ref)


def test_status_2_built_by_hand():
    # a score no y can produce (|u| far beyond the support, which is [-1, 1]): u(beta) > 0 everywhere, 50 clamped steps do not converge
    g, mu = np.array([1.0, -1.0]), np.array([0.5, 0.5])
    lp, st, beta, se, D = GpcaEngine.firth_log10p(g, mu, 10.0)
    ref = firth_reference(g, mu, 10.0)
    assert st == 2 and ref["status"] == 2
    assert lp == GpcaEngine.normal_log10p(10.0 / math.sqrt(0.5)) and beta == pytest.approx(ref["beta"], rel=1e-9) and beta > 100.0
    assert se == pytest.approx(ref["se"], rel=1e-6) and D == pytest.approx(ref["D"], rel=1e-9)
    # no information at 0: g~^2 underflows
    lp, st, beta, se, D = GpcaEngine.firth_log10p(np.array([1e-170, -1e-170]), mu, 0.0)
    assert st == 2 and lp == 0.0 and beta == 0.0 and D == 0.0 and se == INF
    # mu (1 - mu) = 0 everywhere
    lp, st, beta, se, D = GpcaEngine.firth_log10p(g, np.array([0.0, 1.0]), 0.0)
    assert st == 2 and beta == 0.0 and D == 0.0


def test_identity_with_the_offset_model():
    """beta U - K(beta) = l(beta) - l(0) for eta = logit(mu) + beta g~, with mu of a real null fit and g~ = x - X (X^T W X)^-1 X^T W x"""
    rng = np.random.default_rng(11)
    n, Pc = 257, 3
    Cm = rng.standard_normal((n, Pc))
    y = (rng.random(n) < 1 / (1 + np.exp(-(-1.5 + 0.7 * Cm[:, 0])))).astype(np.float64)
    alpha, mu, _ = GpcaEngine.logistic_null(y, Cm)
    X = np.column_stack([np.ones(n), Cm])
    x = rng.integers(0, 3, n).astype(np.float64)
    w = mu * (1 - mu)
    g = x - X @ np.linalg.solve(X.T @ (w[:, None] * X), X.T @ (w * x))
    assert np.max(np.abs(X.T @ (w * g))) < 1e-10
    U = float(g @ (y - mu))
    L = np.longdouble
    gl, ml, yl = g.astype(L), mu.astype(L), y.astype(L)
    eta0 = np.log(ml / (1 - ml))
    ll = lambda b: np.sum(yl * (eta0 + b * gl) - np.log1p(np.exp(eta0 + b * gl)))
    for b in (-2.0, -0.3, 1e-3, 0.5, 3.0):
        K = float(np.sum(firth_terms(g, mu, b)[0]))
        lhs, rhs = b * U - K, float(ll(L(b)) - ll(L(0)))
        scale = float(np.sum(np.abs(yl * b * gl)) + np.sum(np.abs(firth_terms(g, mu, b)[0])))
        assert abs(lhs - rhs) <= (n + 8) * EPS * (scale + abs(b * U)) * 4, (b, lhs, rhs)
    # and the library's D is twice the penalised ratio at its beta^
    lp, st, beta, se, D = GpcaEngine.firth_log10p(g, mu, U)
    t = firth_terms(g, mu, beta)
    pen = 0.5 * math.log(float(np.sum(t[2])) / float(np.sum(w * g * g)))
    assert st == 1 and D == pytest.approx(2 * (float(ll(L(beta)) - ll(L(0))) + pen), rel=1e-9)


# ------------------------------------------------------------------------------------------------ 2. calibration
CALIBRATION = (4.6286, 4.4946, 5.0500, 3.7068)


def test_calibration_rows():
    for i, (x, y) in enumerate(calibration_rows()):
        exact, u, g, mu = exact_log10p(x, y)
        muv = np.full(x.size, mu)
        got = GpcaEngine.firth_log10p(g, muv, u)
        ref = firth_reference(g, muv, u)
        spa = GpcaEngine.spa_log10p(g, muv, u)[0]
        z = u / math.sqrt(float(np.sum(mu * (1 - mu) * g * g)))
        print(f"row {i}: z {z:.2f}  exact {exact:.3f}  Firth {got[0]:.3f} (restatement {ref['log10p']:.3f}, beta {got[2]:.3f}, se {got[3]:.3f}, "
              f"passes {ref['passes']})  SPA {spa:.3f}  normal {GpcaEngine.normal_log10p(z):.2f}")
        assert got[1] == 1
        check_item(got, g, muv, u, ref)
        assert abs(ref["log10p"] - CALIBRATION[i]) <= 0.002 and abs(got[0] - exact) <= 0.4 < 3.0 < GpcaEngine.normal_log10p(z) - exact


# ------------------------------------------------------------------------------------------------ the rule under sanitizers, stand-alone
def test_rule_in_a_program_of_its_own(tmp_path):
    """tests/cpp/firth_math_check.cpp: spa_math.h's rule in a stand-alone host program (g++, no HIP, no library loaded into python):
    240 random vectors, the hand-built failures and the terms at |a| past 710.  It is the program to build with
    -fsanitize=address,undefined -fno-sanitize-recover=all for a sanitizer run (DESIGN.md section 7 records one); here it is built
    plain, so that the suite does not depend on a sanitizer runtime."""
    exe = str(tmp_path / "firth_math_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "genomic_pca_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "firth_math_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("firth_math_check: 240 runs") and last.endswith(" 0 failures"), last


# ------------------------------------------------------------------------------------------------ the ABI's argument rules
def test_firth_log10p_argument_rules():
    lib = _lib.load()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    g, mu, out = np.array([1.0, -1.0]), np.array([0.5, 0.5]), np.zeros(5)
    BA = _lib.GPCA_ERR_BAD_ARG
    assert lib.gpca_firth_log10p(vp(g), vp(mu), 2, 0.25, vp(out)) == 0 and out[1] == 1.0 and out[0] > 0
    assert lib.gpca_firth_log10p(None, vp(mu), 2, 0.25, vp(out)) == BA
    assert lib.gpca_firth_log10p(vp(g), None, 2, 0.25, vp(out)) == BA
    assert lib.gpca_firth_log10p(vp(g), vp(mu), 0, 0.25, vp(out)) == BA
    assert lib.gpca_firth_log10p(vp(g), vp(mu), 2, 0.25, None) == BA
    for bad_u in (math.nan, INF):
        assert lib.gpca_firth_log10p(vp(g), vp(mu), 2, bad_u, vp(out)) == BA
    for bad_mu in (-0.1, 1.1, math.nan):
        assert lib.gpca_firth_log10p(vp(g), vp(np.array([0.5, bad_mu])), 2, 0.25, vp(out)) == BA
    assert lib.gpca_firth_log10p(vp(np.array([1.0, math.inf])), vp(mu), 2, 0.25, vp(out)) == BA
    with pytest.raises(_lib.GpcaError):
        gpca_pkg.firth_log10p(g, np.array([0.5, 2.0]), 0.25)
    # mu = 0 or 1: the sample adds nothing to the sums (it still counts for gmax, which only clamps a step)
    a = gpca_pkg.firth_log10p([1.0, -1.0, 0.5, -0.7], [0.5, 0.5, 0.0, 1.0], 0.25)
    assert a == gpca_pkg.firth_log10p(g, mu, 0.25)
    # U = 0 is corrected like any other score: the penalty alone moves beta where the vector is skewed
    lp, st, beta, se, D = gpca_pkg.firth_log10p([3.0, -1.0, -1.0, -1.0], [0.2, 0.2, 0.2, 0.2], 0.0)
    assert st == 1 and beta != 0.0 and D >= 0.0
