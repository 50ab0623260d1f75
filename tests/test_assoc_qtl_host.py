"""CPU-only: the host side of the many-trait QTL scan (gpca.h section a24).

gpca_qtl_stats against the step-3 formulas of gpca_assoc_linear written in numpy f64 on a table of values that includes rss = 0 and
rss < 0 (division and square root are correctly rounded on both sides, so the values are compared bit for bit); gpca_qtl_t_min, the
bisection that turns a threshold on -log10 p into one on |t|, against gpca_student_t_log10p itself: the result reaches the threshold and
the double below it does not (1 ulp of the monotone search); io.assoc_qtl_bands, io.qtl_best_merge and the two writers, and their
formats.hpp twins through a small compiled driver that must give the same bands and byte-identical files."""
import math
import os
import subprocess

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import io as gio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_qtl_stats_is_the_linear_scan_step_3():
    rng = np.random.default_rng(1)
    xb = np.r_[rng.standard_normal(200) * 10.0, 2.0, 3.0, 0.0, 1e-200]
    sxx = np.r_[rng.uniform(1e-4, 0.05, 40), rng.uniform(0.1, 500.0, 160), 4.0, 4.0, 1.0, 1e-100]       # (the first 40: mostly rss < 0)
    yy = np.r_[rng.uniform(0.5, 400.0, 200), 1.0, 2.0, 5.0, 1.0]                    # [200]: rss = 1 - 2 * 0.5 = 0; [201]: rss = 2 - 2.25 < 0
    df = 97.0
    got = gpca.qtl_stats(xb, sxx, yy, df)
    with np.errstate(all="ignore"):
        beta = xb / sxx
        rss = yy - xb * beta
        se = np.sqrt(rss / df / sxx)
        t = beta / se
    dead = ~(rss > 0.0)
    assert dead[200] and dead[201] and dead[:200].sum() > 0 and (~dead[:200]).sum() > 50
    ref = np.stack([np.where(dead, np.nan, beta), np.where(dead, np.nan, se), np.where(dead, np.nan, t)], 1)
    assert np.array_equal(got, ref, equal_nan=True)
    assert got[202, 0] == 0.0 and got[202, 2] == 0.0 and np.isfinite(got[203]).all()


@pytest.mark.parametrize("df", [1.0, 3.0, 10.0, 97.0, 1012.0, 9988.0, 5e5])
@pytest.mark.parametrize("x", [0.3, 1.0, 5.0, 7.301, 50.0, 300.0])
def test_t_min_is_the_first_t_that_reaches_the_threshold(x, df):
    lp = gpca.GpcaEngine.student_t_log10p
    t = gpca.qtl_t_min(x, df)
    if math.isinf(t):                                    # (df = 1: p falls like 1 / t, a finite t reaches 1e-300 only beyond 1e299)
        assert lp(1.7e308, df) < x
        return
    assert t > 0.0 and lp(t, df) >= x and lp(float(np.nextafter(t, 0.0)), df) < x


def test_t_min_edges():
    assert gpca.qtl_t_min(0.0, 10.0) == 0.0 and gpca.qtl_t_min(-3.0, 10.0) == 0.0
    assert math.isnan(gpca.qtl_t_min(float("nan"), 10.0)) and math.isnan(gpca.qtl_t_min(5.0, 0.0)) and math.isnan(gpca.qtl_t_min(5.0, float("inf")))


def test_bands():
    for K, T, N, cap in ((0, 10, 100, 1000), (1, 1, 1, 0), (1000, 8192, 1000, 1 << 20), (1000000, 8192, 1000, 1 << 20),
                         (1000000, 20000, 500, 1 << 16), (5000, 1 << 20, 100000, 1 << 24), (100000, 100, 1000, 50)):
        b = gio.assoc_qtl_bands(K, T, N, cap)
        assert (not b and K == 0) or (b[0][0] == 0 and b[-1][1] == K)
        for (r0, r1), (s0, _) in zip(b, b[1:] + [(K, K)]):
            assert r1 == s0 and r0 < r1 and r0 % 128 == 0                            # whole row blocks, in order, nothing left out
            rows = r1 - r0
            assert rows <= 128 or (rows * T <= max(cap, 1) * gio.QTL_HITS_PER_PAIRS and rows * N * T <= gio.QTL_BAND_WORK_MAX)


def test_best_merge_keeps_the_lower_row_on_a_tie():
    b2, bw = np.full(4, np.nan), np.full(4, -1, np.int64)
    gio.qtl_best_merge(b2, bw, [0.5, np.nan, 0.25, 0.0], [3, -1, 7, 0])
    gio.qtl_best_merge(b2, bw, [0.5, np.nan, 0.5, 0.0], [130, -1, 131, 128])
    gio.qtl_best_merge(b2, bw, [0.75, 0.125, np.nan, 0.0], [300, 301, -1, 256])
    assert np.array_equal(b2, [0.75, 0.125, 0.5, 0.0]) and np.array_equal(bw, [300, 301, 131, 0])


def test_writers_and_their_twins(tmp_path):
    exe = str(tmp_path / "dump_assoc_qtl")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "genomic_pca_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp", "dump_assoc_qtl.cpp"), "-lz", "-o", exe])
    pre_c, pre_p = str(tmp_path / "c" / "out"), str(tmp_path / "p" / "out")
    lines = subprocess.run([exe, pre_c], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    nan = float("nan")
    # the bands and the merge
    for ln in (l for l in lines if l.startswith("B ")):
        f = ln.split()
        K, T, N, cap = (int(v) for v in f[1:5])
        assert [tuple(int(v) for v in b.split(":")) for b in f[5:]] == gio.assoc_qtl_bands(K, T, N, cap), ln
    assert sum(l.startswith("B ") for l in lines) == 9
    assert [l for l in lines if l.startswith("M ")] == ["M 0.75 300", "M 0.125 301", "M 0.5 131", "M 0 0"]
    # the files
    hits = gio.write_qtl_hits(pre_p, ["1"], [100], ["rs1"], ["A"], ["geneA"], [500.0], [0.25], [1.5], [0.5], [3.0], [2.56789012])
    gio.write_qtl_hits(pre_p, ["1", "X"], [2500000, 7], ["rs2", "rs3"], ["G", "T"], ["geneB", "geneA"], [499.0, 12.0], [0.123456789, 0.5],
                       [-2.5e-7, nan], [1e-7, nan], [-2.5, nan], [1234.5678, nan], append=True)
    best = gio.write_qtl_best(pre_p, ["geneA", "geneB", "geneC"], ["1", None, "22"], [100, 0, 123456789], ["rs1", None, "rs9"], ["A", None, "C"],
                              [1.5, nan, nan], [0.5, nan, nan], [3.0, nan, nan], [2.56789012, nan, nan], [1000, 0, 7])
    assert hits == pre_p + ".qtl.hits" and best == pre_p + ".qtl.best"
    for suffix in (".qtl.hits", ".qtl.best"):
        with open(pre_p + suffix, "rb") as fp, open(pre_c + suffix, "rb") as fc:
            assert fp.read() == fc.read(), suffix
    text = open(hits).read().split("\n")
    assert text[0] == "#CHROM\tPOS\tID\tA1\tTRAIT\tOBS_CT\tA1_FREQ\tBETA\tSE\tT_STAT\tLOG10P"
    assert text[2] == "1\t2500000\trs2\tG\tgeneB\t499\t0.123457\t-2.5e-07\t1e-07\t-2.5\t1234.57" and text[3].endswith("\t0.5\tNA\tNA\tNA\tNA")
    tb = open(best).read().split("\n")
    assert tb[0] == "#TRAIT\tCHROM\tPOS\tID\tA1\tBETA\tSE\tT_STAT\tLOG10P\tN_TESTS" and tb[2] == "geneB\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\t0"
    with pytest.raises(ValueError):
        gio.write_qtl_hits(pre_p, ["1"], [1, 2], ["a"], ["A"], ["g"], [1.0], [0.1], [0.0], [1.0], [0.0], [0.0])
