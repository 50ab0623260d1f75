"""CPU-only: the host rules of cis-QTL mapping (include/gpca.h section a25): the permutation table, the beta approximation, the
windows, the bands and the writer.  No GPU: these entry points run on the host alone."""
import math
import os

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import GpcaEngine, GpcaError, _lib, io
from _admix_cv import philox

STREAM_QTL_PERM = 0x51544C50
LN10 = math.log(10.0)


def perm_table_np(seed, n, P):
    """a25's table: row p = Fisher-Yates from the top, step s (i = n - 1 - s) driven by word s & 3 of philox(counter = (s >> 2, p, 0,
    stream), key = the seed's words); j = (r (i + 1)) >> 32"""
    out = np.zeros((P, n), np.uint32)
    calls = np.arange((max(n - 1, 0) + 3) // 4, dtype=np.uint64)
    for p in range(P):
        w = philox(calls, np.full_like(calls, p), 0, STREAM_QTL_PERM, seed & 0xffffffff, (seed >> 32) & 0xffffffff).reshape(-1)
        a = np.arange(n, dtype=np.uint32)
        for s in range(n - 1):
            i = n - 1 - s
            j = (int(w[s]) * (i + 1)) >> 32
            a[i], a[j] = a[j], a[i]
        out[p] = a
    return out


@pytest.mark.parametrize("seed", [0, 7, (5 << 32) | 9])
def test_perm_table_is_the_philox_restatement(seed):
    for n, P in ((1, 3), (2, 5), (5, 4), (64, 3), (257, 2)):
        got = gpca.qtl_perm_table(seed, n, P)
        assert got.dtype == np.uint32 and got.shape == (P, n)
        assert np.array_equal(got, perm_table_np(seed, n, P)), (n, P)
        assert np.array_equal(np.sort(got, axis=1), np.broadcast_to(np.arange(n, dtype=np.uint32), (P, n)))
    # a row is a function of (seed, row): a shorter table is a prefix
    assert np.array_equal(gpca.qtl_perm_table(seed, 100, 2), gpca.qtl_perm_table(seed, 100, 6)[:2])


def test_perm_table_depends_on_the_seed_and_the_row_and_refuses_bad_sizes():
    a, b = gpca.qtl_perm_table(0, 300, 8), gpca.qtl_perm_table(1, 300, 8)
    assert (a == b).mean() < 0.05
    assert all((a[0] == a[p]).mean() < 0.05 for p in range(1, 8))
    assert gpca.qtl_perm_table(0, 0, 3).shape == (3, 0) and gpca.qtl_perm_table(0, 9, 0).shape == (0, 9)
    with pytest.raises(GpcaError) as ei:
        gpca.qtl_perm_table(0, 5, 65536)
    assert ei.value.status == _lib.GPCA_ERR_BAD_ARG


# ---- the beta approximation ------------------------------------------------------------------------------------------------------------
DF = 200.0


def log10p_of_r2(r2, d):
    return np.array([GpcaEngine.student_t_log10p(math.sqrt(d * x / (1.0 - x)), d) for x in np.asarray(r2, np.float64).ravel()])


def r2_of_log10p(l10p, d):
    t = np.array([GpcaEngine.qtl_t_min(x, d) for x in np.asarray(l10p, np.float64).ravel()])
    return t * t / (t * t + d)


@pytest.fixture(scope="module")
def beta_case():
    rng = np.random.default_rng(20240611)
    p = rng.beta(1.03, 37.0, 10000)
    r2 = r2_of_log10p(-np.log10(p), DF)
    nominal = float(np.quantile(r2, 0.9))
    return r2, nominal, gpca.qtl_beta_approx(r2, nominal, DF)


def digamma_np(x):
    """psi(x), x > 0: the recurrence up to x >= 20, then four terms of the asymptotic series (error below 1e-17)"""
    r = 0.0
    while x < 20.0:
        r -= 1.0 / x
        x += 1.0
    f = 1.0 / (x * x)
    return r + math.log(x) - 0.5 / x - f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f / 132))))


def shape1_mom_np(r2, d):
    p = 10.0 ** -log10p_of_r2(r2, d)
    m, v = p.mean(), p.var(ddof=1)
    return m * (m * (1.0 - m) / v - 1.0)


def test_beta_approx_shapes_satisfy_the_likelihood_equations(beta_case):
    r2, nominal, res = beta_case
    assert res["status"] == 0
    a, b = res["shape1"], res["shape2"]
    p = 10.0 ** -log10p_of_r2(r2, res["true_df"])
    assert abs(digamma_np(a) - digamma_np(a + b) - np.log(p).mean()) < 1e-9
    assert abs(digamma_np(b) - digamma_np(a + b) - np.log1p(-p).mean()) < 1e-9
    # the draws were Beta(1.03, 37) p-values at df = 200: the fit finds them again (10 000 draws: a few per cent)
    assert abs(a - 1.03) < 0.06 and abs(b - 37.0) < 3.0 and abs(res["true_df"] - DF) < 0.1 * DF
    assert res["shape1_mom"] == pytest.approx(shape1_mom_np(r2, res["true_df"]), rel=1e-9)
    assert res["log10p_nominal_true"] == pytest.approx(float(log10p_of_r2([nominal], res["true_df"])[0]), rel=1e-12)


def test_beta_approx_true_df_is_the_root_of_a_dense_search(beta_case):
    r2, _, res = beta_case
    sub = r2[:2000]                                          # (the dense search evaluates 2 000 p-values per point)
    got = gpca.qtl_beta_approx(sub, 0.01, DF)["true_df"]
    # coarse grid, then refine around the sign change
    lo, hi = 1.0, 2.0 * DF
    for _ in range(4):
        grid = np.linspace(lo, hi, 41)
        f = np.array([math.log(shape1_mom_np(sub, d)) for d in grid])
        k = int(np.nonzero(np.sign(f[:-1]) != np.sign(f[1:]))[0][0])
        lo, hi = grid[k], grid[k + 1]
    # (400 / 40^4 = 1.6e-4: far inside 1e-5 df = 2e-3)
    assert abs(got - 0.5 * (lo + hi)) < 1e-5 * DF


def test_beta_approx_log10p_beta_against_scipy(beta_case):
    sp = pytest.importorskip("scipy.special")
    r2, _, res0 = beta_case
    for q in (0.1, 0.5, 0.9, 0.999, 1.0):
        nominal = float(np.quantile(r2, q)) if q < 1.0 else 0.6
        res = gpca.qtl_beta_approx(r2, nominal, DF)
        x = 10.0 ** -res["log10p_nominal_true"]
        want = sp.betainc(res["shape1"], res["shape2"], x)
        if want > 1e-300:
            assert res["log10p_beta"] == pytest.approx(-math.log10(want), rel=1e-9), q


def test_beta_approx_log_space_value_does_not_underflow(beta_case):
    r2, _, _ = beta_case
    nominal = float(r2_of_log10p([200.0], DF)[0])            # a nominal p-value near 1e-200
    res = gpca.qtl_beta_approx(r2, nominal, DF)
    a, b = res["shape1"], res["shape2"]
    logx = -res["log10p_nominal_true"] * LN10
    assert -480.0 < logx < -440.0
    lead = a * logx - math.log(a) - (math.lgamma(a) + math.lgamma(b) - math.lgamma(a + b))   # a log x - log(a B(a, b))
    assert math.isfinite(res["log10p_beta"])
    assert -res["log10p_beta"] * LN10 == pytest.approx(lead, rel=1e-6)
    assert res["pval_perm"] == 1.0 / 10001.0


def test_beta_approx_counting_rule_nan_handling_and_status_bits():
    r2 = np.array([0.01, 0.02, 0.02, 0.03, 0.05, 0.05, 0.05, 0.08, 0.1, 0.2, 0.3, 0.4])
    # ties count: perm_r2 >= r2_nominal
    assert gpca.qtl_beta_approx(r2, 0.05, 50.0)["pval_perm"] == (1 + 8) / 13
    assert gpca.qtl_beta_approx(r2, 0.0500001, 50.0)["pval_perm"] == (1 + 5) / 13
    assert gpca.qtl_beta_approx(r2, 0.5, 50.0)["pval_perm"] == 1 / 13
    # NaN entries drop out of the count and of P
    with_nan = np.concatenate([r2, [np.nan, np.nan]])
    a, b = gpca.qtl_beta_approx(with_nan, 0.05, 50.0), gpca.qtl_beta_approx(r2, 0.05, 50.0)
    assert a == b
    # fewer than 10 left: pval_perm alone
    few = gpca.qtl_beta_approx(np.concatenate([r2[:9], [np.nan] * 5]), 0.02, 50.0)
    assert few["pval_perm"] == (1 + 8) / 10 and few["status"] == 0
    assert all(math.isnan(few[k]) for k in ("true_df", "shape1", "shape2", "log10p_nominal_true", "log10p_beta", "shape1_mom"))
    none = gpca.qtl_beta_approx(np.zeros(0), 0.02, 50.0)
    assert none["pval_perm"] == 1.0 and math.isnan(none["shape1"])
    assert all(math.isnan(v) for k, v in gpca.qtl_beta_approx(r2, float("nan"), 50.0).items() if k != "status")
    # bit 1: p-values far too concentrated for any d in [1, 2 df] (shape1_mom > 1 everywhere): no sign change, d = df
    tight = np.full(50, 0.02) + 1e-6 * np.arange(50)
    res = gpca.qtl_beta_approx(tight, 0.02, 50.0)
    assert res["status"] & 1 and res["true_df"] == 50.0
    # bit 2: a permutation r2 of exactly 0 has p = 1, log(1 - p) = -inf: no likelihood fit, the moment estimates come back
    res = gpca.qtl_beta_approx(np.concatenate([[0.0], r2]), 0.05, 50.0)
    assert res["status"] & 2 and res["shape1"] == res["shape1_mom"] and math.isfinite(res["shape2"])


# ---- windows, bands, writer ------------------------------------------------------------------------------------------------------------
def test_cis_windows_on_two_chromosomes():
    chrom = np.array(["1"] * 5 + ["2"] * 4)
    pos = np.array([100, 200, 300, 400, 500, 150, 250, 350, 450])
    win = io.qtl_cis_windows(chrom, pos, ["1", "1", "1", "2", "2", "X", "1"], [300, 50, 900, 250, 10000, 5, 199], 100)
    assert win.dtype == np.int64
    assert win.tolist() == [[1, 4], [0, 1], [5, 5], [5, 8], [9, 9], [0, 0], [0, 2]]
    # before the first SNP of the chromosome / after the last one: empty, lo = hi
    assert io.qtl_cis_windows(chrom, pos, ["1", "2"], [-500, 10 ** 9], 100).tolist() == [[0, 0], [9, 9]]
    assert io.qtl_cis_windows(chrom, pos, [], [], 100).shape == (0, 2)


def test_cis_windows_refuse_unsorted_positions_like_ld_windows():
    chrom = np.array(["1"] * 3)
    with pytest.raises(ValueError) as a:
        io.qtl_cis_windows(chrom, np.array([100, 90, 300]), ["1"], [100], 50)
    with pytest.raises(ValueError) as b:
        io.ld_windows(chrom, np.array([100, 90, 300]), "1kb")
    assert str(a.value).split(": ", 1)[1] == str(b.value).split(": ", 1)[1]                # the same words after the name
    with pytest.raises(ValueError):
        io.qtl_cis_windows(np.array(["1", "2", "1"]), np.array([1, 2, 3]), ["1"], [1], 50)


def test_cis_bands_cover_the_traits_under_the_limit():
    assert io.assoc_qtl_cis_bands(0, 1000) == []
    assert io.assoc_qtl_cis_bands(7, 0) == [(0, 7)]
    for G, P in ((1, 1), (20000, 1000), (20000, 10000), (5, 65535), (33555, 1000)):
        bands = io.assoc_qtl_cis_bands(G, P)
        assert bands[0][0] == 0 and bands[-1][1] == G and all(a[1] == b[0] for a, b in zip(bands, bands[1:]))
        assert all(0 < (b - a) and (b - a) * P * 8 <= 256 << 20 for a, b in bands)
    assert len(io.assoc_qtl_cis_bands(20000, 10000)) == math.ceil(20000 / ((256 << 20) // 80000))


def test_trait_pos_reader_and_writer_rows(tmp_path):
    src = tmp_path / "pos.txt"
    src.write_text("TRAIT CHROM POS\ng1 1 1000\ng3\t2\t5\n")
    tp = io.read_trait_pos(str(src))
    assert tp == {"g1": ("1", 1000), "g3": ("2", 5)}
    bad = tmp_path / "bad.txt"
    bad.write_text("GENE CHR POS\ng1 1 1000\n")
    with pytest.raises(ValueError):
        io.read_trait_pos(str(bad))
    res = {"n_var": np.array([4, 0, 0]), "best_row": np.array([2, -1, -1]), "best_r2": np.array([0.25, np.nan, np.nan]),
           "best_stat": np.array([[3.0, 12.0, 3.0], [np.nan] * 3, [np.nan] * 3]), "perm_r2": np.tile(np.linspace(0.001, 0.2, 40), (3, 1)), "df": 30.0}
    out = tmp_path / "x.qtl.cis"
    io.write_qtl_cis(str(tmp_path / "x"), ["g1", "g2", "g3"], [("1", 1000), None, ("2", 5)], res,
                     ids=["rs0", "rs1", "rs2", "rs3"], var_pos=[10, 20, 30, 40], a1=["A", "C", "G", "T"])
    lines = out.read_text().splitlines()
    assert lines[0] == "#TRAIT\tCHROM\tPOS\tN_VAR\tID\tVAR_POS\tA1\tBETA\tSE\tT_STAT\tLOG10P_NOMINAL\tTRUE_DF\tSHAPE1\tSHAPE2\tPVAL_PERM\tLOG10P_BETA"
    assert len(lines) == 4
    f = lines[1].split("\t")
    assert f[:7] == ["g1", "1", "1000", "4", "rs2", "30", "G"]
    beta, se, t = gpca.qtl_stats(3.0, 12.0, 3.0, 30.0)[0]
    assert f[7:10] == ["%.6g" % beta, "%.6g" % se, "%.6g" % t]
    ba = gpca.qtl_beta_approx(res["perm_r2"][0], 0.25, 30.0)
    assert f[10] == "%.6g" % GpcaEngine.student_t_log10p(t, 30.0) and f[14] == "%.6g" % ba["pval_perm"] and f[15] == "%.6g" % ba["log10p_beta"]
    assert lines[2].split("\t") == ["g2"] + ["NA"] * 15                            # no position
    assert lines[3].split("\t") == ["g3", "2", "5", "0"] + ["NA"] * 12              # a window without a variant
    # nominal only: the beta columns are NA
    res0 = dict(res, perm_r2=np.zeros((3, 0)))
    io.write_qtl_cis(str(tmp_path / "x"), ["g1", "g2", "g3"], [("1", 1000), None, ("2", 5)], res0,
                     ids=["rs0", "rs1", "rs2", "rs3"], var_pos=[10, 20, 30, 40], a1=["A", "C", "G", "T"])
    f = out.read_text().splitlines()[1].split("\t")
    assert f[10] != "NA" and f[11:] == ["NA"] * 5
