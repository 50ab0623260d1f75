"""CPU-only: gpca_ldsc_fit (include/gpca.h section a19) against a numpy restatement of its rule, and the rule against the truth.

THE REFERENCE is ``ldsc_numpy`` below: the seven steps of a19 with numpy's vector operations; its block sums are np.sum (pairwise
summation) where the C function accumulates sequentially, and that is the only difference between the two.

THE BAR.  On the five inputs of this module (seeds 0 .. 4, m = 20 000, N = 5 000, l = 1 + Gamma(2, 15), true intercept 1.08, true h2
0.4, 200 blocks) the largest relative difference between the C function and ``ldsc_numpy`` over the eight estimates (mean chi2,
lambda_GC, intercept, h2, their standard errors, ratio and its standard error) was measured at 6.971e-14 (the ratio, seed 0, whose
denominator mean chi2 - 1 carries the 6.6e-15 of the mean; intercept and h2 agree to 4.5e-15, their standard errors to 1.9e-14, and
lambda_GC is bit-equal).  The bar is 100 x that = 6.971e-12, far inside the 1e-6 the rule allows.

RECOVERY.  The reported intercept and h2 lie within 4 reported standard errors of the truth on all five seeds (the numpy restatement
alone stays within 1.8)."""
import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from genomic_pca_amd._lib import GpcaError

fit = gpca.GpcaEngine.ldsc_fit
BAR = 6.971e-12
M_SNPS, N_SAMPLES, TRUE_A, TRUE_H2, BLOCKS = 20_000, 5_000.0, 1.08, 0.4, 200
ESTIMATES = ("mean_chi2", "lambda_gc", "intercept", "intercept_se", "h2", "h2_se", "ratio", "ratio_se")
_CASES = {}


def make_case(seed):
    """(chi2, ell): chi2_j = (a + N h2 l_j / M) x a chi-square variate with one degree of freedom.  Cached; do not modify."""
    if seed not in _CASES:
        rng = np.random.default_rng(seed)
        ell = 1.0 + rng.gamma(2.0, 15.0, size=M_SNPS)
        chi2 = (TRUE_A + N_SAMPLES * TRUE_H2 * ell / M_SNPS) * rng.standard_normal(M_SNPS) ** 2
        ell.setflags(write=False); chi2.setflags(write=False)
        _CASES[seed] = (chi2, ell)
    return _CASES[seed]


def ldsc_numpy(chi2, ell, n_samples, M, w_ell=None, n_blocks=200, chi2_max=0.0):
    chi2, ell = np.asarray(chi2, np.float64), np.asarray(ell, np.float64)
    w_ell = ell if w_ell is None else np.asarray(w_ell, np.float64)
    use = np.isfinite(chi2) & np.isfinite(ell) & np.isfinite(w_ell)
    if chi2_max > 0:
        with np.errstate(invalid="ignore"):
            use &= chi2 <= chi2_max
    c, l, wl = chi2[use], np.maximum(ell[use], 1.0), np.maximum(w_ell[use], 1.0)
    mu = c.size
    B = min(n_blocks, mu)
    assert B >= 2 and mu >= 3
    edges = [mu * k // B for k in range(B + 1)]
    mean_c = c.sum() / mu
    a, h = 1.0, min(max(M * (mean_c - 1.0) / (n_samples * (l.sum() / mu)), 0.0), 1.0)

    def sums(w):
        cols = (w, w * l, w * l * l, w * c, w * l * c)
        return np.array([[col[edges[k]:edges[k + 1]].sum() for col in cols] for k in range(B)])

    def solve(s):
        det = s[0] * s[2] - s[1] * s[1]
        return (s[2] * s[3] - s[1] * s[4]) / det, (s[0] * s[4] - s[1] * s[3]) / det

    for _ in range(3):
        w = 1.0 / (wl * 2.0 * (a + n_samples * min(max(h, 0.0), 1.0) * l / M) ** 2)
        blk = sums(w)
        tot = blk.sum(axis=0)
        a, b = solve(tot)
        h = b * M / n_samples
    pa, ph = np.empty(B), np.empty(B)
    for k in range(B):
        ak, bk = solve(tot - blk[k])
        pa[k] = B * a - (B - 1) * ak
        ph[k] = B * h - (B - 1) * bk * M / n_samples
    se_a, se_h = np.sqrt(pa.var(ddof=1) / B), np.sqrt(ph.var(ddof=1) / B)
    nan = float("nan")
    return {"m_used": mu, "mean_chi2": mean_c, "lambda_gc": float(np.median(c)) / 0.4549364231195724, "intercept": a, "intercept_se": se_a,
            "h2": h, "h2_se": se_h, "ratio": (a - 1.0) / (mean_c - 1.0) if mean_c > 1.0 else nan,
            "ratio_se": se_a / (mean_c - 1.0) if mean_c > 1.0 else nan, "n_blocks": B}


def rel_diff(got, ref):
    return max(abs(got[k] - ref[k]) / abs(ref[k]) for k in ESTIMATES)


def test_c_function_equals_the_numpy_restatement():
    worst = 0.0
    for seed in range(5):
        chi2, ell = make_case(seed)
        got = fit(chi2, ell, N_SAMPLES, M_SNPS, n_blocks=BLOCKS)
        ref = ldsc_numpy(chi2, ell, N_SAMPLES, M_SNPS, n_blocks=BLOCKS)
        assert got["m_used"] == ref["m_used"] == M_SNPS and got["n_blocks"] == ref["n_blocks"] == BLOCKS
        d = rel_diff(got, ref)
        print(f"seed {seed}: largest relative difference {d:.3e}: " + ", ".join(f"{k} {abs(got[k] - ref[k]) / abs(ref[k]):.1e}" for k in ESTIMATES))
        worst = max(worst, d)
    print(f"largest relative difference over the five seeds: {worst:.3e} (bar {BAR:.1e})")
    assert BAR <= 1e-6
    assert worst <= BAR
    # with weights of their own, a cap on chi2 and a block count that does not divide the rows
    chi2, ell = make_case(1)
    w_ell = np.sqrt(ell) + 3.0
    got = fit(chi2, ell, N_SAMPLES, M_SNPS, w_ell=w_ell, n_blocks=37, chi2_max=30.0)
    ref = ldsc_numpy(chi2, ell, N_SAMPLES, M_SNPS, w_ell=w_ell, n_blocks=37, chi2_max=30.0)
    assert got["m_used"] == ref["m_used"] < M_SNPS and got["n_blocks"] == 37
    assert rel_diff(got, ref) <= BAR


def test_truth_is_recovered_within_four_standard_errors():
    for seed in range(5):
        chi2, ell = make_case(seed)
        got = fit(chi2, ell, N_SAMPLES, M_SNPS, n_blocks=BLOCKS)
        za, zh = (got["intercept"] - TRUE_A) / got["intercept_se"], (got["h2"] - TRUE_H2) / got["h2_se"]
        print(f"seed {seed}: intercept {got['intercept']:.4f} ({got['intercept_se']:.4f}), h2 {got['h2']:.4f} ({got['h2_se']:.4f}): {za:+.2f} and {zh:+.2f} standard errors")
        assert abs(za) <= 4.0 and abs(zh) <= 4.0
        assert 0.0 < got["intercept_se"] < 0.1 and 0.0 < got["h2_se"] < 0.1
        assert got["ratio"] == (got["intercept"] - 1.0) / (got["mean_chi2"] - 1.0) and got["ratio_se"] == got["intercept_se"] / (got["mean_chi2"] - 1.0)


def test_lambda_gc_on_odd_and_even_counts():
    ell = np.array([1.0, 5.0, 2.0, 9.0, 4.0, 7.0])
    chi2 = np.array([0.3, 2.5, 0.1, 4.0, 1.5, 0.9])
    even = fit(chi2, ell, 100.0, 6.0, n_blocks=3)
    assert even["m_used"] == 6 and even["lambda_gc"] == (0.5 * (0.9 + 1.5)) / 0.4549364231195724
    odd = fit(chi2[:5], ell[:5], 100.0, 6.0, n_blocks=3)
    assert odd["m_used"] == 5 and odd["lambda_gc"] == 1.5 / 0.4549364231195724
    assert abs(even["mean_chi2"] - 9.3 / 6.0) < 1e-15
    low = fit(chi2 * 0.1, ell, 100.0, 6.0, n_blocks=3)                     # mean chi2 <= 1: no ratio
    assert low["mean_chi2"] < 1.0 and np.isnan(low["ratio"]) and np.isnan(low["ratio_se"]) and np.isfinite(low["intercept"])


def test_drop_rules():
    chi2, ell = (a.copy() for a in make_case(0))
    chi2, ell = chi2[:3000], ell[:3000]
    base = fit(chi2, ell, N_SAMPLES, M_SNPS, n_blocks=50)
    # rows that do not count, put between the others, leave every number as it was
    c2 = np.insert(chi2, [5, 5, 1000, 2999], [np.nan, np.inf, 3.0, 2.0])
    l2 = np.insert(ell, [5, 5, 1000, 2999], [10.0, 10.0, np.nan, -np.inf])
    got = fit(c2, l2, N_SAMPLES, M_SNPS, n_blocks=50)
    assert got == base
    w = np.insert(ell, [5, 5, 1000, 2999], [1.0, 1.0, 1.0, 1.0])
    w[7] = np.nan                                                          # a NaN weight drops its row too
    got = fit(c2, l2, N_SAMPLES, M_SNPS, w_ell=w, n_blocks=50)
    assert got["m_used"] == 2999
    # chi2_max: rows above it go, a row at it stays; 0 and None mean no cap
    cap = float(np.sort(chi2)[-11])
    capped = fit(chi2, ell, N_SAMPLES, M_SNPS, n_blocks=50, chi2_max=cap)
    assert capped["m_used"] == 2990
    keep = chi2 <= cap
    assert capped == fit(chi2[keep], ell[keep], N_SAMPLES, M_SNPS, n_blocks=50)
    assert fit(chi2, ell, N_SAMPLES, M_SNPS, n_blocks=50, chi2_max=0.0) == base
    # more blocks than rows: B = m_used
    few = fit(chi2[:40], ell[:40], N_SAMPLES, M_SNPS, n_blocks=200)
    assert few["n_blocks"] == 40 and few["m_used"] == 40


def test_null_weights_equal_the_ld_scores_bit_for_bit():
    chi2, ell = make_case(3)
    a = fit(chi2, ell, N_SAMPLES, M_SNPS, n_blocks=BLOCKS)
    b = fit(chi2, ell, N_SAMPLES, M_SNPS, w_ell=ell.copy(), n_blocks=BLOCKS)
    assert a == b
    c = fit(chi2, ell, N_SAMPLES, M_SNPS, w_ell=np.sqrt(ell) + 3.0, n_blocks=BLOCKS)       # (other weights are read: the answer moves)
    assert c["intercept"] != a["intercept"]


def test_every_bad_argument():
    chi2, ell = make_case(0)
    chi2, ell = chi2[:100], ell[:100]
    lib = _lib.load()
    out = np.zeros(10)

    def rc(c=chi2, l=ell, m=None, n=N_SAMPLES, M=float(M_SNPS), B=10, o=out):
        c, l = np.ascontiguousarray(c, np.float64), np.ascontiguousarray(l, np.float64)
        return lib.gpca_ldsc_fit(c.ctypes.data if c.size else None, l.ctypes.data if l.size else None, None, c.size if m is None else m, n, M, B, 0.0,
                                 None if o is None else o.ctypes.data)
    assert rc() == _lib.GPCA_OK
    assert rc(B=1) == _lib.GPCA_ERR_BAD_ARG and rc(B=0) == _lib.GPCA_ERR_BAD_ARG              # fewer than two blocks
    assert rc(c=chi2[:2], l=ell[:2], B=2) == _lib.GPCA_ERR_BAD_ARG                            # fewer than three rows
    assert rc(c=chi2[:3], l=ell[:3], B=3) == _lib.GPCA_OK
    assert rc(c=chi2[:3], l=ell[:3], B=2) == _lib.GPCA_ERR_BAD_ARG                            # a delete-one estimate from one row: no determinant
    bad = chi2.copy(); bad[2:] = np.nan
    assert rc(c=bad) == _lib.GPCA_ERR_BAD_ARG                                                 # ... after the drop rules
    assert rc(n=0.0) == _lib.GPCA_ERR_BAD_ARG and rc(n=-5.0) == _lib.GPCA_ERR_BAD_ARG and rc(n=float("nan")) == _lib.GPCA_ERR_BAD_ARG
    assert rc(M=0.0) == _lib.GPCA_ERR_BAD_ARG and rc(M=-1.0) == _lib.GPCA_ERR_BAD_ARG
    assert rc(l=np.full(100, 7.0)) == _lib.GPCA_ERR_BAD_ARG                                   # constant l: no determinant
    assert rc(l=np.linspace(-3.0, 0.9, 100)) == _lib.GPCA_ERR_BAD_ARG                         # ... after max(l, 1)
    assert rc(o=None) == _lib.GPCA_ERR_BAD_ARG and rc(m=-1) == _lib.GPCA_ERR_BAD_ARG
    assert rc(c=np.zeros(0), l=np.zeros(0)) == _lib.GPCA_ERR_BAD_ARG
    with pytest.raises(GpcaError):
        fit(chi2, np.full(100, 7.0), N_SAMPLES, M_SNPS)
    with pytest.raises(ValueError):
        fit(chi2, ell[:50], N_SAMPLES, M_SNPS)
