"""CPU-only: the host rules of include/gpca.h section a23 (gpca_fstat_blocks, gpca_fstat) and the readers and writers around them
(io.fstat_blocks, io.read_fstats_list, io.fstat_quad, io.write_f2_summary, io.write_fstats and their twins in host/formats.hpp).

``fstat_restate`` restates steps 1 - 5 of the header independently: the coefficients as exact fractions in a dictionary, the totals as
Python integers, the jackknife in numpy.  The library is held to it at rtol 1e-12.  With equal-sized blocks the weighted jackknife is
the plain delete-one jackknife (rtol 1e-10).  With no group ever missing every pair of a statistic sees the same SNPs, so theta is the
per-SNP mean of the statistic up to the 2^-40 grid (``GRID_BAR``, derived below).  What it is for: the simulation of
tests/_fstat_sim.py, where f3 finds the admixed population, the tree's f4 is zero and the wrong tree's f4 is not.

The sums the tests feed to gpca_fstat come from ``test_gpu_f2_blocks.model_f2``, the numpy model the device is held to bit for bit."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from genomic_pca_amd import io as gio
from genomic_pca_amd._lib import GpcaError

from _fstat_sim import POPS, simulate
from test_gpu_f2_blocks import model_f2, pair_index
from test_gpu_group_counts import model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
fstat = gpca.GpcaEngine.fstat
# theta against the per-SNP mean, no group missing: a pair's sum is off by at most 2^-41 per SNP (the rounding to the grid), so its mean
# is off by at most 2^-41; a statistic has at most four pair terms, each times 1/2: 4 x 1/2 x 2^-41 = 2^-40.  The model adds its per-SNP
# values with math.fsum (one rounding) and forms each value from four v with |v| <= 1.5 in three additions, the library rounds once per
# product, quotient and sum of at most four terms: 32 roundings of values below 4 cover both, 32 x 4 x 2^-53 = 2^-46.
GRID_BAR = 2.0 ** -40 + 2.0 ** -46


# ------------------------------------------------------------------------------------------------ the header's steps, restated
def fstat_restate(acc, cnt, quad):
    acc, cnt = np.asarray(acc), np.asarray(cnt)
    B = acc.shape[0]
    a, b, c, d = quad
    coef = {}
    for (x, y), s in (((a, d), 1), ((b, c), 1), ((a, c), -1), ((b, d), -1)):
        if x != y:
            i, j = max(x, y), min(x, y)
            q = i * (i - 1) // 2 + j
            coef[q] = coef.get(q, Fraction(0)) + Fraction(s, 2)
    coef = {q: float(v) for q, v in sorted(coef.items()) if v != 0}
    if not coef:
        return [math.nan] * 6
    qs = list(coef)
    used = [blk for blk in range(B) if all(cnt[blk, q] >= 1 for q in qs)]
    G = len(used)
    S = {q: sum(int(acc[blk, q]) for blk in used) for q in qs}
    C = {q: sum(int(cnt[blk, q]) for blk in used) for q in qs}
    minc = min(C.values())
    if G < 2:
        return [math.nan] * 4 + [float(G), float(minc)]
    theta = sum(coef[q] * ((float(S[q]) * 2.0 ** -40) / float(C[q])) for q in qs)
    tm = np.array([sum(coef[q] * ((float(S[q] - int(acc[blk, q])) * 2.0 ** -40) / float(C[q] - int(cnt[blk, q]))) for q in qs) for blk in used])
    m = np.array([float(sum(int(cnt[blk, q]) for q in qs)) for blk in used])
    n = m.sum()
    h = n / m
    tj = G * theta - np.sum((n - m) / n * tm)
    tau = h * theta - (h - 1.0) * tm
    var = np.sum((tau - tj) ** 2 / (h - 1.0)) / G
    se = math.sqrt(var)
    return [theta, tj, se, theta / se, float(G), float(minc)]


def random_blocks(B, P, seed, holes=True):
    """acc and cnt as a panel would give them: counts of 30 .. 80 SNPs, f2 near 0.01 with noise; some (block, pair) entries empty"""
    rng = np.random.default_rng(seed)
    pairs = P * (P - 1) // 2
    cnt = rng.integers(30, 80, (B, pairs)).astype(np.int64)
    per = rng.normal(0.01, 0.004, (B, pairs)) * rng.uniform(0.2, 3.0, pairs)
    if holes:
        cnt[rng.random((B, pairs)) < 0.1] = 0
    acc = np.rint(per * cnt * 2.0 ** 40).astype(np.int64)
    return acc, cnt


def all_quads(P, rng, k=40):
    return [tuple(int(x) for x in rng.integers(0, P, 4)) for _ in range(k)]


def test_fstat_against_the_restated_steps():
    rng = np.random.default_rng(5)
    for P, B, seed in ((2, 7, 1), (3, 12, 2), (5, 40, 3), (64, 9, 4)):
        acc, cnt = random_blocks(B, P, seed)
        quads = all_quads(P, rng) + [(0, 1, 0, 1), (1, 0, 1, 0), (0, 1, 1, 0), (P - 1, 0, P - 1, 0)]
        if P >= 3:
            quads += [(2, 0, 2, 1), (0, 1, 0, 2), (2, 2, 0, 1), (0, 0, 1, 2)]
        got = fstat(acc, cnt, quads)
        assert got.shape == (len(quads), 6)
        for g, q in zip(got, quads):
            want = fstat_restate(acc, cnt, q)
            np.testing.assert_allclose(g, want, rtol=1e-12, atol=0.0, equal_nan=True, err_msg=str(q))
    # f2 is symmetric, f4 changes sign when one side is swapped, and f3(C; A, B) is symmetric in A and B
    acc, cnt = random_blocks(20, 4, 9, holes=False)
    r = fstat(acc, cnt, [(0, 1, 0, 1), (1, 0, 1, 0), (0, 1, 2, 3), (1, 0, 2, 3), (2, 0, 2, 1), (2, 1, 2, 0)])
    assert np.array_equal(r[0], r[1]) and np.array_equal(r[4], r[5])
    assert r[2][0] == -r[3][0] and r[2][2] == r[3][2] and r[2][3] == -r[3][3]
    assert (r[0][0] > 0) and r[0][4] == 20


def test_equal_blocks_give_the_delete_one_jackknife():
    B, P = 25, 4
    acc, cnt = random_blocks(B, P, 11, holes=False)
    cnt[:] = 57
    for quad in ((0, 1, 0, 1), (2, 0, 2, 1), (0, 1, 2, 3)):
        theta, tj, se, z, G, minc = fstat(acc, cnt, [quad])[0]
        assert G == B and minc == 57 * B
        per_pair = acc / 2.0 ** 40 / cnt                      # block means; equal counts: the totals' mean is their mean

        def stat(pp):
            f2 = lambda x, y: 0.0 if x == y else pp[max(x, y) * (max(x, y) - 1) // 2 + min(x, y)]
            a, b, c, d = quad
            return 0.5 * (f2(a, d) + f2(b, c) - f2(a, c) - f2(b, d))
        full = stat(per_pair.mean(0))
        loo = np.array([stat(np.delete(per_pair, k, 0).mean(0)) for k in range(B)])
        np.testing.assert_allclose(theta, full, rtol=1e-10)
        np.testing.assert_allclose(tj, B * full - (B - 1) * loo.mean(), rtol=1e-10)
        np.testing.assert_allclose(se, math.sqrt((B - 1) / B * np.sum((loo - loo.mean()) ** 2)), rtol=1e-10)
        np.testing.assert_allclose(z, theta / se, rtol=1e-10)


def complete_counts(M, P, n, seed):
    """counts [M][P][3] of P groups of n samples with every call observed, the groups' frequencies scattered around a per-SNP one"""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.05, 0.95, (M, 1))
    p = np.clip(base + rng.normal(0, 0.08, (M, P)), 0.01, 0.99)
    g = (rng.random((M, P, n)) < p[..., None]).astype(np.int64) + (rng.random((M, P, n)) < p[..., None]).astype(np.int64)
    return np.stack([np.full((M, P), n), (g == 1).sum(-1), (g == 2).sum(-1)], -1).astype(np.uint32)


def test_theta_is_the_per_snp_mean_when_no_group_is_missing():
    M, P, n = 3000, 5, 12
    counts = complete_counts(M, P, n, 21)
    block = (np.arange(M) // 100).astype(np.int32)
    acc, cnt, q, ok = model_f2(counts, block, 30, want_q=True)
    assert ok.all() and (cnt == 100).all()
    # the per-SNP v in f64, as the chain forms it
    I, J = pair_index(P)
    c = counts.astype(np.float64)
    nn = 2.0 * c[..., 0]
    p = (c[..., 1] + 2.0 * c[..., 2]) / nn
    h = (p * (1.0 - p)) / (nn - 1.0)
    d = p[:, I] - p[:, J]
    v = (d * d - h[:, I]) - h[:, J]
    assert np.abs(v).max() <= 1.5 and np.abs(q - v * 2.0 ** 40).max() <= 0.5

    def f2(x, y):
        return np.zeros(M) if x == y else v[:, max(x, y) * (max(x, y) - 1) // 2 + min(x, y)]
    quads = [(0, 1, 0, 1), (3, 4, 3, 4), (2, 0, 2, 1), (4, 1, 4, 3), (0, 1, 2, 3), (0, 2, 1, 3), (4, 0, 1, 2), (0, 1, 1, 2)]
    got = fstat(acc, cnt, quads)
    worst = 0.0
    for g, (a, b, cc, dd) in zip(got, quads):
        per_snp = 0.5 * (((f2(a, dd) + f2(b, cc)) - f2(a, cc)) - f2(b, dd))
        direct = math.fsum(per_snp) / M
        worst = max(worst, abs(g[0] - direct))
        assert g[4] == 30 and g[5] == M
    print(f"max |theta - per-SNP mean| = {worst:.3e}, bar {GRID_BAR:.3e}")
    assert worst <= GRID_BAR


def test_fewer_than_two_blocks_and_empty_statistics():
    acc, cnt = random_blocks(6, 3, 31, holes=False)
    cnt[1:, 0] = 0                                           # pair (1, 0) lives in block 0 only
    r = fstat(acc, cnt, [(0, 1, 0, 1), (0, 0, 0, 0), (1, 1, 0, 2), (0, 2, 0, 2), (0, 1, 1, 0)])
    assert np.isnan(r[0][:4]).all() and r[0][4] == 1 and r[0][5] == cnt[0, 0]        # G = 1
    assert np.isnan(r[1]).all() and np.isnan(r[2]).all()                             # no non-zero coefficient
    assert np.isfinite(r[3]).all() and r[3][4] == 6
    # f4(0, 1; 1, 0) = 1/2 [f2(0, 0) + f2(1, 1) - 2 f2(0, 1)] = -f2(0, 1): the same blocks as f2(0, 1), the sign turned
    assert np.isnan(r[4][:4]).all() and r[4][4] == 1
    cnt[:, 0] = 0                                            # ... in no block at all
    r = fstat(acc, cnt, [(0, 1, 0, 1)])[0]
    assert np.isnan(r[:4]).all() and r[4] == 0 and r[5] == 0
    cnt[:, 0] = 40
    r = fstat(acc, cnt, [(0, 1, 1, 0), (0, 1, 0, 1)])
    assert r[0][0] == -r[1][0] and r[0][2] == r[1][2]


def test_fstat_bad_arguments():
    lib = _lib.load()
    import ctypes
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    acc, cnt = random_blocks(4, 3, 41)
    quads, out = np.array([[0, 1, 0, 1]], np.int32), np.zeros((1, 6))
    call = lambda a, c, B, P, q, M, o: lib.gpca_fstat(vp(a), vp(c), B, P, vp(q), M, vp(o))
    assert call(acc, cnt, 4, 3, quads, 1, out) == _lib.GPCA_OK
    for bad in ((None, cnt, 4, 3, quads, 1, out), (acc, None, 4, 3, quads, 1, out), (acc, cnt, 4, 3, None, 1, out), (acc, cnt, 4, 3, quads, 1, None),
                (acc, cnt, 0, 3, quads, 1, out), (acc, cnt, 4, 1, quads, 1, out), (acc, cnt, 4, 65, quads, 1, out), (acc, cnt, 4, 3, quads, -1, out),
                (acc, cnt, 4, 3, np.array([[0, 1, 0, 3]], np.int32), 1, out), (acc, cnt, 4, 3, np.array([[0, -1, 0, 1]], np.int32), 1, out)):
        assert call(*bad) == _lib.GPCA_ERR_BAD_ARG, bad[2:6]
    assert call(acc, cnt, 4, 3, None, 0, out) == _lib.GPCA_OK                        # no statistic asked for
    with pytest.raises(GpcaError):
        fstat(acc, cnt, [(0, 1, 0, 3)])
    with pytest.raises(ValueError):
        fstat(acc[:, :2], cnt[:, :2], [(0, 1, 0, 1)])                                # 2 is not a number of pairs


def test_fstat_blocks():
    # a chromosome change starts a block, whatever the block holds
    b, B = gio.fstat_blocks(["1", "1", "chr1", "2", "2", "2", "X"], [10, 20, 30, 5, 6, 7, 1], "5")
    assert B == 3 and b.dtype == np.int32 and list(b) == [0, 0, 0, 1, 1, 1, 2]
    # the N-th row: a block of N rows is full
    b, B = gio.fstat_blocks(["1"] * 7, [1] * 7, "3")
    assert list(b) == [0, 0, 0, 1, 1, 1, 2] and B == 3
    b, B = gio.fstat_blocks(["1"] * 4 + ["2"] * 3, list(range(7)), "2")
    assert list(b) == [0, 0, 1, 1, 2, 2, 3] and B == 4
    # the kb boundary: pos - first = N 1000 starts the next block, one less does not; the span is counted from the block's first row
    b, B = gio.fstat_blocks(["1"] * 6, [100, 5099, 5100, 10099, 10100, 10101], "5kb")
    assert list(b) == [0, 0, 1, 1, 2, 2] and B == 3
    b, B = gio.fstat_blocks(["1"] * 3 + ["2"] * 2, [0, 4999, 5000, 5000, 9999], "5KB")
    assert list(b) == [0, 0, 1, 2, 2] and B == 3
    b, B = gio.fstat_blocks(["7"] * 3, [1, 2, 3])                                    # the default: 5000kb
    assert list(b) == [0, 0, 0] and B == 1 and gio.FSTAT_BLOCK_DEFAULT == "5000kb"
    b, B = gio.fstat_blocks([], [], "500")
    assert b.shape == (0,) and B == 0
    for bad in ("", "kb", "0kb", "1", "-3", "5 mb"):
        with pytest.raises(ValueError):
            gio.fstat_blocks(["1"], [1], bad)
    # the C function itself
    import ctypes
    lib = _lib.load()
    nb = ctypes.c_int32(-1)
    ch, pos, blk = np.array([0, 0, 1, 0], np.uint8), np.array([1, 2, 3, 4], np.int64), np.zeros(4, np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.gpca_fstat_blocks(vp(ch), None, 4, 3, _lib.FSTAT_BLOCK_VARIANTS, vp(blk), ctypes.byref(nb)) == _lib.GPCA_OK
    assert list(blk) == [0, 0, 1, 1] and nb.value == 2
    assert lib.gpca_fstat_blocks(vp(ch), None, 4, 3, _lib.FSTAT_BLOCK_BP, vp(blk), ctypes.byref(nb)) == _lib.GPCA_ERR_BAD_ARG
    assert lib.gpca_fstat_blocks(vp(ch), vp(pos), 4, 0, _lib.FSTAT_BLOCK_BP, vp(blk), ctypes.byref(nb)) == _lib.GPCA_ERR_BAD_ARG
    assert lib.gpca_fstat_blocks(vp(ch), vp(pos), 4, 3, 2, vp(blk), ctypes.byref(nb)) == _lib.GPCA_ERR_BAD_ARG
    assert lib.gpca_fstat_blocks(vp(ch), vp(pos), -1, 3, 0, vp(blk), ctypes.byref(nb)) == _lib.GPCA_ERR_BAD_ARG
    assert lib.gpca_fstat_blocks(None, vp(pos), 4, 3, 0, vp(blk), ctypes.byref(nb)) == _lib.GPCA_ERR_BAD_ARG
    assert lib.gpca_fstat_blocks(None, None, 0, 3, 0, None, ctypes.byref(nb)) == _lib.GPCA_OK and nb.value == 0


LIST = """# the tests of the panel
f2 EUR AFR

f3 ADM EUR AFR
  f4 EUR AFR EAS ADM
#f2 nobody nothing
f2 AFR AFR
"""
NAMES = ["EUR", "AFR", "EAS", "ADM"]


def test_list_reader_and_writers(tmp_path):
    path = tmp_path / "list.txt"
    path.write_text(LIST)
    lst = gio.read_fstats_list(str(path), NAMES)
    assert lst == [("f2", (0, 1)), ("f3", (3, 0, 1)), ("f4", (0, 1, 2, 3)), ("f2", (1, 1))]
    assert [gio.fstat_quad(k, g) for k, g in lst] == [(0, 1, 0, 1), (3, 0, 3, 1), (0, 1, 2, 3), (1, 1, 1, 1)]
    for text, msg in (("f5 EUR AFR\n", ":1: 'f5' is not f2, f3 or f4"), ("f2 EUR AFR\nf3 EUR AFR\n", ":2: f3 takes 3 groups, 2 are given"),
                      ("\nf4 EUR AFR EAS ADM EUR\n", ":2: f4 takes 4 groups, 5 are given"), ("f2 EUR SAS\n", ":1: no group 'SAS' in the within file")):
        path.write_text(text)
        with pytest.raises(ValueError) as ei:
            gio.read_fstats_list(str(path), NAMES)
        assert str(ei.value) == str(path) + msg
    with pytest.raises(ValueError):
        gio.fstat_quad("f3", (0, 1))
    nan = math.nan
    stats = np.array([[0.0123456789, 0.0124, 0.00051, 24.2072, 40, 19876], [-0.006, -0.0061, 0.0001, -60.0, 39, 500],
                      [nan, nan, nan, nan, 1, 12], [nan] * 6])
    lines = open(gio.write_fstats(str(tmp_path / "o" / "P"), NAMES, lst, stats)).read().split("\n")
    assert lines == ["#STAT\tPOP1\tPOP2\tPOP3\tPOP4\tEST\tSE\tZ\tN_BLOCKS\tN_SNPS", "f2\tEUR\tAFR\t.\t.\t0.0123457\t0.00051\t24.2072\t40\t19876",
                     "f3\tADM\tEUR\tAFR\t.\t-0.006\t0.0001\t-60\t39\t500", "f4\tEUR\tAFR\tEAS\tADM\tNA\tNA\tNA\t1\t12",
                     "f2\tAFR\tAFR\t.\t.\tNA\tNA\tNA\tNA\tNA", ""]
    s3 = np.array([[0.01, 0.01, 0.001, 10.0, 5, 100], [nan, nan, nan, nan, 0, 0], [1e-7, 1e-7, 2.5e-8, 4.0, 2, 7]])
    lines = open(gio.write_f2_summary(str(tmp_path / "o" / "P"), NAMES[:3], s3)).read().split("\n")
    assert lines == ["#POP1\tPOP2\tF2\tSE\tZ\tN_BLOCKS\tN_SNPS", "EUR\tAFR\t0.01\t0.001\t10\t5\t100", "EUR\tEAS\tNA\tNA\tNA\t0\t0",
                     "AFR\tEAS\t1e-07\t2.5e-08\t4\t2\t7", ""]
    with pytest.raises(ValueError):
        gio.write_f2_summary(str(tmp_path / "o" / "Q"), NAMES, s3)
    with pytest.raises(ValueError):
        gio.write_fstats(str(tmp_path / "o" / "Q"), NAMES, lst, s3)


def test_formats_hpp_writes_the_same_bytes(tmp_path):
    gpca.load()
    pkg = os.path.join(ROOT, "genomic_pca_amd")
    exe = str(tmp_path / "dump_fstats")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(pkg, "host"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "dump_fstats.cpp"), "-o", exe, "-L" + pkg, "-lgpca", "-lz", "-Wl,-rpath," + pkg])
    P, B, K = 4, 9, 23
    acc, cnt = random_blocks(B, P, 51)
    cnt[1:, 5] = 0                                                                        # pair (3, 2) lives in one block: NA
    chrom = ["1"] * 9 + ["chr1"] * 3 + ["2"] * 11
    pos = [1000 * i for i in range(12)] + [500 + 2500 * i for i in range(11)]
    data, lst = tmp_path / "d.txt", tmp_path / "list.txt"
    with open(data, "w") as f:
        f.write(f"{K} {P} {B}\n" + " ".join(NAMES) + "\n")
        f.writelines(f"{c} {p}\n" for c, p in zip(chrom, pos))
        f.write(" ".join(str(int(v)) for v in acc.ravel()) + "\n" + " ".join(str(int(v)) for v in cnt.ravel()) + "\n")
    lst.write_text(LIST + "f2 EAS ADM\nf4 ADM EAS EUR AFR\n")
    items = gio.read_fstats_list(str(lst), NAMES)
    for spec in ("4", "5kb", "2.5kb", "5000kb"):
        pre = str(tmp_path / ("c_" + spec) / "P")
        r = subprocess.run([exe, pre, str(lst), spec, str(data)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        b, nb = gio.fstat_blocks(chrom, pos, spec)
        out = r.stdout.splitlines()
        assert out[0] == f"blocks {nb}:" + "".join(f" {int(x)}" for x in b)
        assert out[1:] == [k + "".join(f" {g}" for g in gs) + " -> " + " ".join(str(x) for x in gio.fstat_quad(k, gs)) for k, gs in items]
        want = str(tmp_path / ("py_" + spec) / "P")
        gio.write_f2_summary(want, NAMES, fstat(acc, cnt, [(j, i, j, i) for j, i in gio.fst_pairs(P)]))
        gio.write_fstats(want, NAMES, items, fstat(acc, cnt, [gio.fstat_quad(k, g) for k, g in items]))
        for s in (".f2.summary", ".fstats"):
            got, exp = open(pre + s, "rb").read(), open(want + s, "rb").read()
            assert got == exp and len(got) > 100, s
    assert b"NA" in open(want + ".f2.summary", "rb").read()
    # the refusals carry the same words
    for spec, text in (("0kb", "f2 EUR AFR\n"), ("4", "f3 EUR AFR\n"), ("4", "f2 EUR SAS\n"), ("x", "f9 EUR\n")):
        lst.write_text(text)
        r = subprocess.run([exe, str(tmp_path / "e" / "P"), str(lst), spec, str(data)], capture_output=True, text=True, timeout=60)
        out = r.stdout.splitlines()
        for line, fn in ((out[0], lambda: gio.fstat_blocks(chrom, pos, spec)), (out[-1], lambda: gio.read_fstats_list(str(lst), NAMES))):
            try:
                fn()
                assert not line.startswith("error ")
            except ValueError as e:
                assert line == "error " + str(e)


# ------------------------------------------------------------------------------------------------ what it is for
SIM_SEED = 2012


@pytest.fixture(scope="module")
def sim_blocks():
    G, pop = simulate(SIM_SEED)
    counts = model(G, pop, len(POPS))
    block, B = gio.fstat_blocks(["1"] * G.shape[0], list(range(1, G.shape[0] + 1)), "500")
    assert B == 40
    return model_f2(counts, block, B)


def test_f3_finds_the_admixed_population_and_f4_the_tree(sim_blocks):
    acc, cnt = sim_blocks
    A, B_, C, D, X = range(5)
    f3, f4_tree, f4_wrong, f2_ab, f2_ac = fstat(acc, cnt, [gio.fstat_quad("f3", (X, A, C)), (A, B_, C, D), (A, C, B_, D), (A, B_, A, B_), (A, C, A, C)])
    print(f"f3(X; A, C) = {f3[0]:.6f} Z = {f3[3]:.1f};  f4(A, B; C, D) = {f4_tree[0]:.6f} Z = {f4_tree[3]:.2f};  "
          f"f4(A, C; B, D) = {f4_wrong[0]:.6f} Z = {f4_wrong[3]:.1f};  f2(A, B) = {f2_ab[0]:.5f}, f2(A, C) = {f2_ac[0]:.5f}")
    assert f3[4] == 40 and 19000 < f3[5] <= 20000
    assert f3[3] < -10 and abs(f4_tree[3]) < 4 and f4_wrong[3] > 10
    # the sizes: f3 = -f2(A, C) / 4 in expectation, and f4 of the wrong tree is the inner branches' drift
    assert abs(f3[0] + f2_ac[0] / 4.0) < 5 * f3[2] + 1e-3 and 0 < f2_ab[0] < f2_ac[0]
    # every non-target population: f3 is positive
    others = fstat(acc, cnt, [gio.fstat_quad("f3", (A, B_, C)), gio.fstat_quad("f3", (C, A, D))])
    assert (others[:, 3] > 10).all()
