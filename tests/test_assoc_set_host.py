"""CPU-only: the burden and SKAT rules of one set on the host -- gpca_set_test (include/gpca.h section a16).

This module holds a numpy f64 restatement of section a16's host rule (set_test_reference): the same used-row rule, the same burden
sums, numpy's symmetric eigensolver in place of the library's, the same eigenvalue cut, the same bracketed Newton and the same two
tails.  It is the reference of tests/test_gpu_assoc_set.py as well.  The C function must agree with it in status and to 1e-9 relative
in -log10 p and zeta (the two differ by their eigenvalues' rounding, about 1e-15 relative, and by the stopping rule's 1e-10 ub on
zeta, which moves -log10 p only in second order because d(zeta Q - K) / dzeta = 0 at the root).

Accuracy of the METHOD against an exact reference that needs no quadrature.  For a spectrum whose eigenvalues each occur twice, Q is a
sum of scaled chi^2_2 variables and
    P(Q > q) = sum_k prod_{j != k} lambda_k / (lambda_k - lambda_j) exp(-q / (2 lambda_k)),
evaluated here in 80-digit decimal arithmetic (the products cancel heavily for close eigenvalues).  Phi = O diag(lambda, lambda) O^T
with a random orthogonal O, unit weights, u scaled to the wanted Q = c1 + z_Q sqrt(2 c2).  Spectra: {1, 1/2, 1/4, 1/8, 1/16}, {1, 0.3},
eight values 1 .. 1.35, {1, .01, .02, .03} and a single lambda.  Measured with the restatement (max |value - exact -log10 p|):
    saddle point, z_Q in {0.5, 1, 2, 4, 8, 16, 32} (exact -log10 p up to 31):   0.02349  (the first spectrum at z_Q = 32)
    bulk value,   z_Q in {-1, -0.5, 0, 0.25}:                                  0.02080  (the first spectrum at z_Q = 0.25)
SADDLE_GAP and BULK_GAP are these figures rounded up in the last digit; the C function is asserted at twice them (the convention of WALD_GAP in tests/test_gpu_assoc_score.py)."""
import ctypes as C
import decimal
import math

import numpy as np
import pytest

from genomic_pca_amd import _lib
import genomic_pca_amd as gpca_pkg

LN10 = math.log(10.0)
SADDLE_GAP = 0.02350
BULK_GAP = 0.02081
SPECTRA = {
    "halving": [1.0, 0.5, 0.25, 0.125, 0.0625],
    "two": [1.0, 0.3],
    "close": [1.0 + 0.05 * i for i in range(8)],
    "dominant": [1.0, 0.01, 0.02, 0.03],
    "single": [0.7],
}
ZQ_SADDLE = (0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0)
ZQ_BULK = (-1.0, -0.5, 0.0, 0.25)


# ------------------------------------------------------------------------------------------------ the restatement of section a16
def normal_log10p_two_sided(z):
    z = abs(float(z))
    if z != z:
        return float("nan")
    if z < 37.0:
        return -math.log10(math.erfc(z / math.sqrt(2.0))) if z > 0 else 0.0
    x = z / math.sqrt(2.0)
    s, t = 1.0, 1.0
    for k in range(1, 12):
        t *= -(2 * k - 1) / (2.0 * x * x)
        s += t
    return (x * x + 0.5 * math.log(math.pi) + math.log(x) - math.log(s)) / LN10


def upper_log10p(x):
    """-log10(1 - Phi(x))"""
    if x != x:
        return float("nan")
    if x >= 0.0:
        return normal_log10p_two_sided(x) + math.log10(2.0)
    return -math.log1p(-0.5 * math.erfc(-x / math.sqrt(2.0))) / LN10


def bulk_value(Q, c1, c2):
    kappa, nu = c2 / c1, c1 * c1 / c2
    h = 2.0 / (9.0 * nu)
    return upper_log10p((np.cbrt(Q / (kappa * nu)) - (1.0 - h)) / math.sqrt(h))


def set_test_reference(u, phi, weight=None):
    """section a16's host rule, line by line; phi [m][m] symmetric.  Returns the dict of GpcaEngine.set_test."""
    u, phi = np.asarray(u, np.float64), np.asarray(phi, np.float64)
    m = u.shape[0]
    w = np.ones(m) if weight is None else np.asarray(weight, np.float64)
    d = np.diag(phi)
    with np.errstate(invalid="ignore"):
        used = np.isfinite(u) & np.isfinite(d) & (d > 0) & np.isfinite(w) & (w > 0)
    idx = np.flatnonzero(used)
    nan = float("nan")
    res = dict(m_used=int(idx.size), burden_beta=nan, burden_se=nan, burden_z=nan, burden_log10p=nan, skat_q=nan, skat_log10p=nan,
               skat_status=0, z_q=nan, zeta=nan)
    if idx.size == 0:
        return res
    om = w[idx]
    A = (om[:, None] * phi[np.ix_(idx, idx)]) * om[None, :]
    t = om * u[idx]
    B, v, Q = float(t.sum()), float(A.sum()), float((t * t).sum())
    if v > 0:
        res.update(burden_beta=B / v, burden_se=1 / math.sqrt(v), burden_z=B / math.sqrt(v), burden_log10p=normal_log10p_two_sided(B / math.sqrt(v)))
    res["skat_q"] = Q
    if not np.all(np.isfinite(A)):
        return res
    lam = np.sort(np.linalg.eigvalsh(np.tril(A) + np.tril(A, -1).T))[::-1]
    pos = lam[lam >= 0]
    keep = pos.mean() / 1e5 if pos.size else 0.0
    lam = lam[lam > keep]
    if lam.size == 0:
        return res
    c1, c2 = float(lam.sum()), float((lam * lam).sum())
    zq = (Q - c1) / math.sqrt(2 * c2)
    res["z_q"] = zq
    res["skat_log10p"] = bulk_value(Q, c1, c2)
    if not zq >= 0.5:
        return res
    ub = 1.0 / (2.0 * lam[0])
    lo, hi, zeta = 0.0, ub, (Q - c1) / (2 * c2)
    if not (lo < zeta < hi):
        zeta = 0.5 * (lo + hi)

    def k12(z):
        r = lam / (1.0 - 2.0 * z * lam)
        return float(r.sum()), 2.0 * float((r * r).sum())
    found = False
    for _ in range(200):
        k1, k2 = k12(zeta)
        f = k1 - Q
        if not math.isfinite(f):
            break
        if f > 0:
            hi = zeta
        else:
            lo = zeta
        zn = zeta - f / k2
        if not (lo < zn < hi):
            zn = 0.5 * (lo + hi)
        found = abs(zn - zeta) <= 1e-10 * ub
        zeta = zn
        if found:
            break
    res["zeta"], res["skat_status"] = zeta, 2
    if not found:
        return res
    K = -0.5 * float(np.log1p(-2.0 * zeta * lam).sum())
    k1, k2 = k12(zeta)
    with np.errstate(all="ignore"):
        ww = math.sqrt(2 * (zeta * Q - K)) if zeta * Q - K >= 0 else nan
        vv = zeta * math.sqrt(k2)
        r = ww + math.log(vv / ww) / ww if ww == ww and ww > 0 and vv > 0 else nan
    if not (math.isfinite(r) and r > 0):
        return res
    res["skat_log10p"], res["skat_status"] = upper_log10p(r), 1
    return res


# ------------------------------------------------------------------------------------------------ the exact reference
def exact_log10p(lams, q):
    """-log10 P(sum_k lambda_k chi^2_2 > q) for distinct lambda_k, in 80-digit decimals"""
    with decimal.localcontext() as ctx:
        ctx.prec = 80
        L = [decimal.Decimal(repr(x)) for x in lams]
        qd = decimal.Decimal(repr(float(q)))
        tot = decimal.Decimal(0)
        for k, lk in enumerate(L):
            pr = decimal.Decimal(1)
            for j, lj in enumerate(L):
                if j != k:
                    pr *= lk / (lk - lj)
            tot += pr * (-qd / (2 * lk)).exp()
        return float(-tot.log10())


def doubled_case(lams, zq, seed=3):
    lam2 = np.array(list(lams) * 2, np.float64)
    m = lam2.size
    O, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((m, m)))
    phi = (O * lam2) @ O.T
    phi = 0.5 * (phi + phi.T)
    c1, c2 = lam2.sum(), (lam2 * lam2).sum()
    Q = c1 + (zq + 1e-9) * math.sqrt(2 * c2)          # (a hair above the grid value: 0.5 itself must land on the saddle point's side)
    u = np.full(m, math.sqrt(max(Q, 0.0) / m))
    return u, phi, float(u @ u)


def c_set_test(u, phi, weight=None):
    return gpca_pkg.set_test(u, phi, weight)


def same(a, b):
    """two result dicts agree exactly (NaN equals NaN)"""
    return a.keys() == b.keys() and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


# ------------------------------------------------------------------------------------------------ the tests
def test_c_function_follows_the_restatement():
    rng = np.random.default_rng(11)
    statuses = set()
    for m in (1, 2, 3, 7, 20, 64, 128):
        for scale in (0.3, 1.0, 2.5, 6.0):
            X = rng.standard_normal((m + 5, m)) * rng.uniform(0.2, 2.0, m)
            phi = X.T @ X
            u = rng.standard_normal(m) * np.sqrt(np.diag(phi)) * scale
            wt = rng.uniform(0.5, 25.0, m) if m % 2 else None
            got, ref = c_set_test(u, phi, wt), set_test_reference(u, phi, wt)
            assert got["m_used"] == ref["m_used"] == m and got["skat_status"] == ref["skat_status"], (m, scale, got, ref)
            statuses.add(got["skat_status"])
            for k in ("burden_beta", "burden_se", "burden_z", "burden_log10p", "skat_q", "skat_log10p", "z_q"):
                assert rel(got[k], ref[k]) <= 1e-9 or abs(got[k] - ref[k]) <= 1e-12, (m, scale, k, got[k], ref[k])
            if got["skat_status"] == 1:
                assert rel(got["zeta"], ref["zeta"]) <= 1e-9, (m, scale, got["zeta"], ref["zeta"])
            else:
                assert math.isnan(got["zeta"]) and math.isnan(ref["zeta"])
    assert statuses == {0, 1}


def test_burden_is_the_direct_formula():
    rng = np.random.default_rng(5)
    m = 9
    X = rng.standard_normal((40, m))
    phi, u, w = X.T @ X, rng.standard_normal(m) * 5, rng.uniform(0.1, 3, m)
    got = c_set_test(u, phi, w)
    B, v = float(w @ u), float(w @ phi @ w)
    assert rel(got["burden_z"], B / math.sqrt(v)) < 1e-13 and rel(got["burden_beta"], B / v) < 1e-13
    assert rel(got["burden_se"], 1 / math.sqrt(v)) < 1e-13
    assert rel(got["burden_log10p"], normal_log10p_two_sided(B / math.sqrt(v))) < 1e-12
    assert rel(got["skat_q"], float(((w * u) ** 2).sum())) < 1e-14


@pytest.mark.parametrize("name", sorted(SPECTRA))
def test_accuracy_against_the_exact_tail_of_a_doubled_spectrum(name):
    lams = SPECTRA[name]
    worst_ref = {0: 0.0, 1: 0.0}
    for grid, status, gap in ((ZQ_SADDLE, 1, SADDLE_GAP), (ZQ_BULK, 0, BULK_GAP)):
        for zq in grid:
            u, phi, Q = doubled_case(lams, zq)
            exact = exact_log10p(lams, Q) if Q > 0 else 0.0
            got, ref = c_set_test(u, phi), set_test_reference(u, phi)
            assert got["skat_status"] == ref["skat_status"] == status, (name, zq, got, ref)
            worst_ref[status] = max(worst_ref[status], abs(ref["skat_log10p"] - exact))
            print(f"{name:9s} z_Q={zq:5.2f} exact={exact:9.5f} restatement={ref['skat_log10p']:9.5f} C={got['skat_log10p']:9.5f}")
            assert abs(ref["skat_log10p"] - exact) <= gap, (name, zq, ref["skat_log10p"], exact)   # the docstring's figures hold
            assert abs(got["skat_log10p"] - exact) <= 2 * gap, (name, zq, got["skat_log10p"], exact)
    print(f"{name}: restatement's worst gap: saddle {worst_ref[1]:.5f}, bulk {worst_ref[0]:.5f}")


def test_one_row_is_the_rows_own_test():
    u, phi = np.array([3.1]), np.array([[2.0]])
    got = c_set_test(u, phi)
    z = 3.1 / math.sqrt(2.0)
    assert got["m_used"] == 1 and rel(got["burden_z"], z) < 1e-15
    # SKAT with one row: Q / phi is one chi^2_1, whose upper tail is the two-sided normal value of z
    exact = normal_log10p_two_sided(z)
    assert got["skat_status"] == 1 and abs(got["skat_log10p"] - exact) < 0.05, (got, exact)
    assert rel(got["skat_log10p"], set_test_reference(u, phi)["skat_log10p"]) < 1e-9


def test_rows_that_drop_out():
    rng = np.random.default_rng(2)
    X = rng.standard_normal((30, 5))
    phi, u = X.T @ X, rng.standard_normal(5) * 4
    keep = [0, 2, 4]
    ref = c_set_test(u[keep], phi[np.ix_(keep, keep)])
    w = np.ones(5)
    w[[1, 3]] = 0.0
    assert same(c_set_test(u, phi, w), ref)                                  # a zero weight drops its row
    u2 = u.copy()
    u2[[1, 3]] = np.nan
    assert same(c_set_test(u2, phi), ref)                                    # a NaN u drops its row
    p3 = phi.copy()
    p3[1, :] = p3[:, 1] = np.nan
    p3[3, 3] = 0.0
    assert same(c_set_test(u, p3), ref)                                      # so do a NaN and a zero variance
    none = c_set_test(np.full(5, np.nan), phi)
    assert none["m_used"] == 0 and none["skat_status"] == 0
    assert all(math.isnan(none[k]) for k in none if k not in ("m_used", "skat_status"))


def test_sizes_and_bad_arguments():
    lib = _lib.load()
    rng = np.random.default_rng(4)
    X = rng.standard_normal((200, 128))
    phi, u = X.T @ X, rng.standard_normal(128) * 20
    got, ref = c_set_test(u, phi), set_test_reference(u, phi)
    assert got["m_used"] == 128 and got["skat_status"] == ref["skat_status"] and rel(got["skat_log10p"], ref["skat_log10p"]) < 1e-9
    out = np.zeros(10)
    lo = np.zeros(129 * 130 // 2)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.gpca_set_test(vp(np.ones(129)), vp(lo), None, 129, vp(out)) == _lib.GPCA_ERR_BAD_ARG
    assert lib.gpca_set_test(vp(np.ones(2)), vp(lo), None, 0, vp(out)) == _lib.GPCA_ERR_BAD_ARG
    assert lib.gpca_set_test(None, vp(lo), None, 2, vp(out)) == _lib.GPCA_ERR_BAD_ARG
    assert lib.gpca_set_test(vp(np.ones(2)), vp(lo), None, 2, None) == _lib.GPCA_ERR_BAD_ARG
    for bad in (-1.0, float("nan")):
        assert lib.gpca_set_test(vp(np.ones(2)), vp(np.array([1.0, 0.0, 1.0])), vp(np.array([1.0, bad])), 2, vp(out)) == _lib.GPCA_ERR_BAD_ARG
