"""CPU-only: the host pieces of the logistic score scan -- gpca_logistic_null and gpca_normal_log10p (gpca_assoc_score.cpp), the
helpers of genomic_pca_amd/io.py (binary_trait, assoc_score_groups, assoc_score_bands, write_assoc_logistic) with their twins in
host/formats.hpp, and the rules of --gpca-assoc-logistic in both programs.

gpca_logistic_null against this module's own numpy Newton on the same standardised design X = (1, C centred over the included
samples and scaled to unit norm), iterated until the step is below 1e-14.  The bars: the engine stops when max |delta| <= 1e-10
(1 + max |alpha|), and Newton's next step from there is far smaller, so alpha is held to twice the stopping rule, 2e-10 (1 + max
|alpha|), plus 64 kappa e for the solve (kappa = the condition number of X^T W X, computed here; e = 2^-53); mu = expit(X alpha)
moves by at most |x_n| . d alpha / 4, held to sum_j |x_nj| times the bar of alpha; the gradient X^T (y - mu) of the engine's mu is
(X^T W X) d alpha to first order, held to the bar of alpha times the infinity norm of X^T W X.

gpca_normal_log10p against mpmath at 50 digits, -log10(erfc(|z| / sqrt 2)), on |z| in {0, 1e-3, 1, 5, 37, 40, 200}; the grid reaches
-log10 p = 8 688 (|z| = 200), far past the 308 where p itself underflows.  Largest relative error measured on the grid: 4.1e-16
(|z| = 200); the bar is 8 times that, 3.3e-15, well inside the 1e-9 that six printed digits need."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from genomic_pca_amd import _lib, io as gio
from genomic_pca_amd.cli import main
from genomic_pca_amd.engine import GpcaEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "genomic_pca_amd", "bin", "genomic_pca")
EPS = 2.0 ** -53
WORST = 4.1e-16
BAR = 8 * WORST
assert BAR <= 1e-9
ZS = [0, 1e-3, 1, 5, 37, 40, 200]
SHAPES = [(4, 0), (63, 3), (64, 3), (65, 3), (255, 8), (256, 29), (257, 30), (1023, 61), (1025, 61)]


# ------------------------------------------------------------------------------------------------ gpca_logistic_null
def null_inputs(N, Pc, seed):
    rng = np.random.default_rng(seed)
    Cm = rng.standard_normal((N, Pc))
    n = np.arange(N)
    y = (rng.random(N) < 1.0 / (1.0 + np.exp(-(0.8 * (n % 2) - 0.4)))).astype(np.float64)
    if N == 4:
        y = np.array([0.0, 1.0, 0.0, 1.0])
    inc = np.ones(N, np.uint8)
    if N >= 10:
        inc[3::10] = 0                                 # an excluded tenth carries values no fit could take
        y[inc == 0] = np.where(np.arange(int((inc == 0).sum())) % 2 == 0, 1e30, np.nan)
        Cm[inc == 0] = np.where((np.arange(int((inc == 0).sum())) % 2 == 0)[:, None], np.nan, 1e30)
    return y, Cm, inc


def design(Cm, inc):
    s = inc.astype(bool)
    Cc = Cm[s] - Cm[s].mean(0)
    return np.hstack([np.ones((int(s.sum()), 1)), Cc / np.sqrt((Cc ** 2).sum(0))])


def numpy_newton(X, y):
    """(alpha, steps, converged, max |eta|): Newton from (logit(ybar), 0, ...) until max |delta| < 1e-14"""
    a = np.zeros(X.shape[1])
    a[0] = math.log(y.mean() / (1.0 - y.mean()))
    for it in range(1, 41):
        m = 1.0 / (1.0 + np.exp(-X @ a))
        d = np.linalg.solve(X.T @ ((m * (1 - m))[:, None] * X), X.T @ (y - m))
        a = a + d
        if np.max(np.abs(d)) < 1e-14:
            return a, it, True, float(np.max(np.abs(X @ a)))
    return a, 40, False, float(np.max(np.abs(X @ a)))


@pytest.mark.parametrize("N,Pc", SHAPES)
def test_logistic_null_against_numpy_newton(N, Pc):
    for seed in range(4):
        y, Cm, inc = null_inputs(N, Pc, seed)
        s = inc.astype(bool)
        X = design(Cm, inc)
        ref, steps, conv, eta = numpy_newton(X, y[s])
        assert conv and eta < 30, (N, Pc, seed, steps, eta)                         # the reference converges on every case
        alpha, mu, iters = GpcaEngine.logistic_null(y, Cm, inc)
        m = 1.0 / (1.0 + np.exp(-X @ ref))
        H = X.T @ ((m * (1 - m))[:, None] * X)
        kappa = np.linalg.cond(H)
        bar = 2e-10 * (1 + np.max(np.abs(ref))) + 64 * kappa * EPS
        err = np.max(np.abs(alpha - ref))
        print(f"N={N} Pc={Pc} seed={seed}: engine {iters} steps, numpy {steps}; max |eta| {eta:.2f}; kappa {kappa:.3g}; |d alpha| {err:.2e} of {bar:.2e}")
        assert 1 <= iters <= 25 and err <= bar
        assert np.all(mu[~s] == 0.0)
        assert np.all(np.abs(mu[s] - m) <= np.abs(X).sum(1) * bar)
        assert np.max(np.abs(X.T @ (y[s] - mu[s]))) <= bar * np.linalg.norm(H, np.inf)
        if Pc == 0:
            assert abs(alpha[0] - math.log(y[s].mean() / (1 - y[s].mean()))) <= bar     # the intercept-only fit is logit(ybar)


def test_logistic_null_error_paths():
    lib = _lib.load()
    rng = np.random.default_rng(5)
    N = 120
    y = (rng.random(N) < 0.4).astype(np.float64)
    Cm = rng.standard_normal((N, 3))

    def status(yv, cv, inc=None):
        with pytest.raises(_lib.GpcaError) as ei:
            GpcaEngine.logistic_null(yv, cv, inc)
        return ei.value.status
    BA, NC = _lib.GPCA_ERR_BAD_ARG, _lib.GPCA_ERR_NOT_CONVERGED
    assert GpcaEngine.logistic_null(y, Cm)[2] >= 1
    assert status(np.ones(N), Cm) == BA and status(np.zeros(N), Cm) == BA                # one class
    yh = y.copy(); yh[5] = 0.5
    assert status(yh, Cm) == BA                                                          # y = 0.5
    for v in (np.nan, np.inf, 2.0, -1.0):
        yb = y.copy(); yb[7] = v
        assert status(yb, Cm) == BA
        inc = np.ones(N, np.uint8); inc[7] = 0
        assert GpcaEngine.logistic_null(yb, Cm, inc)[1][7] == 0.0                        # ... but not on an excluded sample
    Cc = Cm.copy(); Cc[:, 1] = 4.0
    assert status(y, Cc) == BA                                                           # a constant column
    Cd = Cm.copy(); Cd[:, 2] = Cd[:, 0]
    assert status(y, Cd) == BA                                                           # a duplicated column
    Cn = Cm.copy(); Cn[3, 0] = np.nan
    assert status(y, Cn) == BA
    few = np.zeros(N, np.uint8); few[:4] = 1
    ya = y.copy(); ya[:4] = [0, 1, 0, 1]
    assert status(ya, Cm, few) == BA                                                     # n - Pc - 1 = 0
    assert status((Cm[:, 0] > 0).astype(np.float64), Cm) == NC                           # a perfectly separating covariate
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    a, m = np.zeros(4), np.zeros(N)
    assert lib.gpca_logistic_null(None, vp(Cm), 3, None, N, vp(a), vp(m), None) == BA
    assert lib.gpca_logistic_null(vp(y), None, 3, None, N, vp(a), vp(m), None) == BA
    assert lib.gpca_logistic_null(vp(y), vp(Cm), -1, None, N, vp(a), vp(m), None) == BA
    assert lib.gpca_logistic_null(vp(y), vp(Cm), 3, None, N, vp(a), vp(m), None) == 0   # iters may be NULL


# ------------------------------------------------------------------------------------------------ gpca_normal_log10p
def test_normal_log10p_against_mpmath():
    import mpmath as mp
    f = _lib.load().gpca_normal_log10p
    worst, top = 0.0, 0.0
    with mp.workdps(50):
        for z in ZS:
            got = f(float(z))
            assert got == f(-float(z)) == GpcaEngine.normal_log10p(-float(z))
            if z == 0:
                assert got == 0.0
                continue
            ref = -mp.log10(mp.erfc(mp.mpf(z) / mp.sqrt(2)))
            rel = float(abs((mp.mpf(got) - ref) / ref))
            worst, top = max(worst, rel), max(top, float(ref))
            assert rel <= BAR, (z, got, float(ref), rel)
    print("largest relative error on the grid", worst, "largest -log10 p", top)
    assert top > 308
    assert math.isnan(f(float("nan"))) and f(float("inf")) == float("inf")


# ------------------------------------------------------------------------------------------------ the helpers of io.py
def test_binary_trait_rules():
    nan = float("nan")
    assert np.array_equal(gio.binary_trait([0, 1, 1, 0]), [0, 1, 1, 0])
    assert np.array_equal(gio.binary_trait([1, 2, 2, 1]), [0, 1, 1, 0])                  # plink's coding: 2 = case
    assert np.array_equal(gio.binary_trait([1, nan, 2, 1]), [0, nan, 1, 0], equal_nan=True)
    assert np.array_equal(gio.binary_trait([nan, 0.0, 1.0]), [nan, 0, 1], equal_nan=True)
    for v in ([0, 1, 2], [1, 1, 1], [0, 0], [2, 2], [0, 2], [0, 1, 0.5], [-1, 1], [nan, nan], [], [0, 1, float("inf")], [1, 2, 3]):
        assert gio.binary_trait(v) is None, v


def test_assoc_score_groups_and_bands():
    assert gio.assoc_score_groups(1, 0) == [(0, 1)]
    assert gio.assoc_score_groups(21, 0) == [(0, 21)] and gio.assoc_score_groups(22, 0) == [(0, 21), (21, 22)]
    assert gio.assoc_score_groups(50, 0) == [(0, 21), (21, 42), (42, 50)]
    assert gio.assoc_score_groups(5, 10) == [(0, 4), (4, 5)]
    assert gio.assoc_score_groups(3, 29) == [(0, 2), (2, 3)] and gio.assoc_score_groups(2, 30) == [(0, 1), (1, 2)]
    assert gio.assoc_score_groups(7, 61) == [(i, i + 1) for i in range(7)] and gio.assoc_score_groups(0, 4) == []
    with pytest.raises(ValueError, match="more than 64 columns"):
        gio.assoc_score_groups(1, 62)
    for T, Pc in ((1, 0), (21, 0), (4, 13), (1, 61)):
        for a, b in gio.assoc_score_groups(T, Pc):
            assert 1 <= (b - a) * (Pc + 3) <= 64
    assert gio.assoc_score_bands(0, 1, 0) == []
    assert gio.assoc_score_bands(10, 4, 13, max_values=256) == gio.assoc_bands(10, 64, 256) == [(0, 4), (4, 8), (8, 10)]
    assert gio.assoc_score_bands(3000000, 4, 13) == gio.assoc_bands(3000000, 64)


def test_write_assoc_logistic_against_a_literal_file(tmp_path):
    prefix = str(tmp_path / "out" / "run")
    nan = float("nan")
    path = gio.write_assoc_logistic(prefix, "cad", ["1", "1", "X"], [100, 2500000, 7], ["rs1", "rs2", "rs3"], ["A", "G", "T"],
                                    [500.0, 499.0, 0.0], [0.25, 0.123456789, nan], [1.5, -2.5e-7, nan], [0.5, 1e-7, nan], [3.0, -2.5, nan],
                                    [2.56789012, 1234.5678, nan])
    assert path == prefix + ".cad.assoc.logistic"
    gio.write_assoc_logistic(prefix, "cad", ["2"], [9], ["rs4"], ["C"], [12.0], [0.5], [1e10], [123456789.0], [0.0], [0.0], append=True)
    want = ("#CHROM\tPOS\tID\tA1\tOBS_CT\tA1_FREQ\tBETA\tSE\tZ_STAT\tLOG10P\n"
            "1\t100\trs1\tA\t500\t0.25\t1.5\t0.5\t3\t2.56789\n"
            "1\t2500000\trs2\tG\t499\t0.123457\t-2.5e-07\t1e-07\t-2.5\t1234.57\n"
            "X\t7\trs3\tT\t0\tNA\tNA\tNA\tNA\tNA\n"
            "2\t9\trs4\tC\t12\t0.5\t1e+10\t1.23457e+08\t0\t0\n")
    assert open(path).read() == want
    with pytest.raises(ValueError):
        gio.write_assoc_logistic(prefix, "t2d", ["1"], [1, 2], ["a"], ["A"], [1], [1], [1], [1], [1], [1])


def _write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return str(path)


def test_cpp_twins_match_python(tmp_path):
    """formats.hpp against io.py: binary_trait on the columns of tables, the groups, the bands, the writer's bytes"""
    exe = str(tmp_path / "dump_assoc_score")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "genomic_pca_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp", "dump_assoc_score.cpp"), "-lz", "-o", exe])
    files = [_write(tmp_path / "a.pheno", "FID IID cc12 cc01 q one na12 half big\n"
                                          "f0 s0 1 0 0.5 1 NA 0 0\nf1 s1 2 1 1 1 1 1 1\nf2 s2 2 NA 2 1 2 0.5 2\nf3 s3 1 0 0 1 nan 1 1\n"),
             _write(tmp_path / "b.pheno", "#FID IID inf01 allna zero2\nf0 s0 0 NA 0\nf1 s1 1 NA 2\nf2 s2 inf NA 0\n")]
    want = []
    for p in files:
        t = gio.read_pheno(p)
        cells = []
        for j, name in enumerate(t.names):
            b = gio.binary_trait(t.values[:, j])
            cells.append(f"{name}:-" if b is None else f"{name}:{'%g' % (np.nanmin(t.values[:, j]) - np.nanmin(b))}")
        want.append(" ".join(["T", *cells]))
    assert want[0] == "T cc12:1 cc01:0 q:- one:- na12:1 half:- big:-" and want[1] == "T inf01:- allna:- zero2:-"
    for T, Pc in ((1, 0), (21, 0), (22, 0), (50, 0), (5, 10), (3, 29), (2, 30), (7, 61), (0, 4)):
        want.append(" ".join([f"G {T} {Pc}", *(f"{a}:{b}" for a, b in gio.assoc_score_groups(T, Pc))]))
    try:
        gio.assoc_score_groups(1, 62)
    except ValueError as e:
        want.append(f"E {e}")
    for K, T, Pc in ((0, 1, 0), (10, 21, 0), (200000000, 1, 61), (3000000, 4, 13)):
        want.append(" ".join(["B", *(f"{a}:{b}" for a, b in gio.assoc_score_bands(K, T, Pc))]))
    want += [f"b {a}:{b}" for a, b in gio.assoc_score_bands(10, 4, 13, 256)]
    pre_c, pre_p = str(tmp_path / "c" / "run"), str(tmp_path / "p" / "run")
    out = subprocess.run([exe, pre_c, *files], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[:-1] == want
    nan = float("nan")
    gio.write_assoc_logistic(pre_p, "cad", ["1", "1", "X", "2"], [100, 2500000, 7, 9], ["rs1", "rs2", "rs3", "rs4"], ["A", "G", "T", "C"],
                             [500.0, 499.0, 0.0, 12.0], [0.25, 0.123456789, nan, 0.5], [1.5, -2.5e-7, nan, 1e10], [0.5, 1e-7, nan, 123456789.0],
                             [3.0, -2.5, nan, 0.0], [2.56789012, 1234.5678, nan, float("inf")])
    assert open(pre_c + ".cad.assoc.logistic", "rb").read() == open(pre_p + ".cad.assoc.logistic", "rb").read()


# ------------------------------------------------------------------------------------------------ the flag of both command lines
BASE = ["--bed-file", "t.bed", "--ld-block-file", "l.txt", "--out", "x"]


def pheno_files(d):
    ids = [f"f{i} s{i}" for i in range(6)]
    return {
        "mixed": _write(d / "mixed.pheno", "FID IID cc height\n" + "".join(f"{s} {1 + i % 2} {i * i}\n" for i, s in enumerate(ids))),
        "quant": _write(d / "quant.pheno", "FID IID t1 t2\n" + "".join(f"{s} {i} {i * i}\n" for i, s in enumerate(ids))),
        # 60 case / control columns and 6 quantitative ones
        "wide": _write(d / "wide.pheno", "FID IID " + " ".join(f"b{j}" for j in range(60)) + " " + " ".join(f"q{j}" for j in range(6)) + "\n" +
                       "".join(s + "".join(f" {(i + j) % 2}" for j in range(60)) + "".join(f" {i * (j + 1)}" for j in range(6)) + "\n"
                               for i, s in enumerate(ids))),
        "cov": _write(d / "cov.txt", "FID IID age sex batch\n" + "".join(f"{s} 4{i} {i % 2} {i % 3}\n" for i, s in enumerate(ids))),
    }


def bad_flags(f):
    """(flags, message) for every refusal that --gpca-assoc-logistic adds and that needs no device"""
    E = ["--eigensnp", "--gpca-assoc-logistic", "--gpca-assoc-pheno"]
    return [
        (["--eigensnp", "--gpca-assoc-logistic"], "--gpca-assoc-logistic needs --gpca-assoc-pheno"),
        (["--gpca-assoc-logistic", "--gpca-assoc-pheno", f["mixed"]], "--gpca-assoc-pheno needs the --eigensnp workflow"),
        # Pc + 3 > 64 where a column is binary: 62 PCs; 59 PCs + 3 covariates
        (E + [f["mixed"], "--eigensnp-k-global", "62"], "--gpca-assoc-logistic: 62 PCs + 0 covariates + 3 are more than 64 columns"),
        (E + [f["mixed"], "--eigensnp-k-global", "59", "--gpca-assoc-covar", f["cov"]],
         "--gpca-assoc-logistic: 59 PCs + 3 covariates + 3 are more than 64 columns"),
        (E + [f["wide"], "--eigensnp-k-global", "60", "--gpca-assoc-covar", f["cov"]], "--gpca-assoc-logistic: 60 PCs + 3 covariates + 3"),
        # the 64-column check of the linear scan counts the quantitative traits only: 6 + 56 + 3 = 65 (and 56 + 3 + 3 = 62 is fine)
        (E + [f["wide"], "--eigensnp-k-global", "61", "--gpca-assoc-pcs", "56", "--gpca-assoc-covar", f["cov"]],
         "--gpca-assoc-pheno: 6 traits + 56 PCs + 3 covariates are more than 64 columns"),
        # without the flag every column is a trait of the linear scan, as before
        (["--eigensnp", "--gpca-assoc-pheno", f["wide"]], "66 traits + 10 PCs + 0 covariates are more than 64 columns"),
        # the refusals of the linear scan hold with the flag
        (E + [f["mixed"], "--gpca-stream", "on"], "--gpca-assoc-pheno needs the genotype matrix resident on the device"),
        (E + [f["mixed"], "--gpca-assoc-vif", "0.5"], "--gpca-assoc-vif must be finite and at least 1"),
        (E + [f["mixed"], "--gpca-eigensnp-local-stage"], "--gpca-assoc-pheno cannot be combined with --gpca-eigensnp-local-stage"),
    ]


def test_flag_errors_python(tmp_path):
    f = pheno_files(tmp_path)
    for flags, msg in bad_flags(f):
        with pytest.raises(SystemExit) as ei:
            main(BASE + flags)
        assert str(ei.value).startswith("error: ") and msg in str(ei.value), (flags, str(ei.value))
    # accepted flags get as far as the missing fileset: 60 binary + 6 quantitative traits with 10 PCs; no binary column and 62 PCs
    for ok in (["--gpca-assoc-pheno", f["wide"]], ["--gpca-assoc-pheno", f["quant"], "--eigensnp-k-global", "62"],
               ["--gpca-assoc-pheno", f["mixed"], "--eigensnp-k-global", "58", "--gpca-assoc-covar", f["cov"]]):
        with pytest.raises(FileNotFoundError) as ei:
            main(BASE + ["--eigensnp", "--gpca-assoc-logistic"] + ok)
        assert "t.fam" in str(ei.value) or "t.bed" in str(ei.value), str(ei.value)


def test_flag_errors_cpp(tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "genomic_pca_amd", "host"), "-s"])
    f = pheno_files(tmp_path)
    for flags, msg in bad_flags(f):
        r = subprocess.run([BIN, *BASE, *flags], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stderr.startswith("error: ") and msg in r.stderr, (flags, r.stderr)
        with pytest.raises(SystemExit) as ei:                                          # the same text from the Python command line
            main(BASE + flags)
        assert str(ei.value) + "\n" == r.stderr
    assert "--gpca-assoc-logistic" in subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
