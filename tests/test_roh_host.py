"""CPU-only: the host side of the runs of homozygosity (include/gpca.h section a20): io.roh_breaks, io.roh_bands, io.roh_select and
io.roh_summary against plain-Python restatements of their rules; the C rule gpca_roh_select against io.roh_select, at equality of both
bounds; the exact bytes of a small P.hom and P.hom.indiv, NA included; and the fraction rule of the window threshold."""
import ctypes
import math

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from genomic_pca_amd import io as gio
from genomic_pca_amd.engine import GpcaEngine


def test_roh_breaks_against_its_rule():
    rng = np.random.default_rng(1)
    chroms = ["1"] * 7 + ["chr2"] * 5 + ["X"] + ["3"] * 4
    pos = np.concatenate([np.sort(rng.integers(1, 5000, n)) for n in (7, 5, 1, 4)])
    pos[3] = pos[2]                                                                  # equal positions are in order
    for gap in (0, 1, 300, 1000, 10 ** 9):
        want, prev = [], None
        for j, c in enumerate(chroms):
            if c != prev:
                want.append(3)
            else:
                want.append(2 if int(pos[j]) - int(pos[j - 1]) > gap else 0)
            prev = c
        got = gio.roh_breaks(chroms, pos, gap)
        assert got.dtype == np.uint8 and got.tolist() == want, gap
    assert gio.roh_breaks(chroms, pos, 10 ** 9).tolist().count(3) == 4 and gio.roh_breaks([], [], 5).shape == (0,)
    # a gap exactly at the limit does not break; one bp more does
    assert gio.roh_breaks(["1", "1", "1"], [10, 1010, 2011], 1000).tolist() == [3, 0, 2]
    with pytest.raises(ValueError, match="reappears at variant 3"):
        gio.roh_breaks(["1", "2", "2", "1"], [1, 1, 2, 5], 10)
    with pytest.raises(ValueError, match="position of variant 2"):
        gio.roh_breaks(["1", "1", "1"], [5, 9, 8], 10)
    with pytest.raises(ValueError, match="one position per"):
        gio.roh_breaks(["1", "1"], [5], 10)
    # the same complaints as ld_windows, word for word behind the function's name
    for args in ((["1", "2", "2", "1"], [1, 1, 2, 5]), (["1", "1", "1"], [5, 9, 8])):
        with pytest.raises(ValueError) as a:
            gio.roh_breaks(*args, 10)
        with pytest.raises(ValueError) as b:
            gio.ld_windows(*args, "5")
        assert str(a.value).replace("roh_breaks", "X") == str(b.value).replace("ld_windows", "X")


def test_roh_bands_cut_only_at_domain_starts():
    rng = np.random.default_rng(2)
    for trial in range(60):
        K = int(rng.integers(1, 120))
        brk = np.where(rng.random(K) < 0.15, 3, np.where(rng.random(K) < 0.2, 2, 0)).astype(np.uint8)
        brk[0] = rng.choice([0, 3])                                                  # (row 0 starts a domain whatever it holds)
        starts = [0] + [j for j in range(1, K) if brk[j] & 1] + [K]
        for max_rows in (1, 7, 30, 1000):
            bands = gio.roh_bands(brk, max_rows)
            assert bands[0][0] == 0 and bands[-1][1] == K and all(a[1] == b[0] for a, b in zip(bands[:-1], bands[1:]))
            for r0, r1 in bands:
                assert r0 in starts and r1 in starts and r1 > r0
                inside = [s for s in starts if r0 < s < r1]
                assert r1 - r0 <= max_rows or not inside                             # longer than the limit: one domain
            for (r0, r1), (_, n1) in zip(bands[:-1], bands[1:]):                      # greedy: the next domain did not fit
                nxt = min(s for s in starts if s > r1)
                assert nxt - r0 > max_rows and n1 >= nxt
    assert gio.roh_bands(np.zeros(0, np.uint8)) == [] and gio.roh_bands(np.array([3, 0, 2, 3, 0], np.uint8)) == [(0, 5)]


def random_records(rng, K, n, N):
    first = rng.integers(0, K, n)
    last = np.minimum(first + rng.integers(0, 40, n), K - 1)
    return np.stack([rng.integers(0, N, n), first, last, rng.integers(0, 3, n), rng.integers(0, 3, n)], 1).astype(np.uint32)


def test_roh_select_and_the_c_rule():
    rng = np.random.default_rng(3)
    K, N = 400, 9
    pos = np.cumsum(rng.integers(1, 3000, K)).astype(np.int64)
    segs = random_records(rng, K, 300, N)
    lib = _lib.load()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for min_bp, dens in ((0, 0), (0, 10 ** 12), (20000, 1500), (5000, 1400), (1, 1)):
        want = np.array([1 if (int(pos[l]) - int(pos[f]) >= min_bp and int(pos[l]) - int(pos[f]) <= dens * (int(l) - int(f) + 1)) else 0
                         for _, f, l, _, _ in segs], np.uint8)
        got = gio.roh_select(segs, pos, min_bp, dens)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (min_bp, dens)
        keep = np.full(len(segs), 9, np.uint8)
        assert lib.gpca_roh_select(vp(segs), len(segs), vp(pos), min_bp, dens, vp(keep)) == _lib.GPCA_OK
        assert np.array_equal(keep, want) and np.array_equal(GpcaEngine.roh_select(segs, pos, min_bp, dens), want)
        assert 0 < want.sum() < len(want) or (min_bp, dens) in ((0, 0), (0, 10 ** 12), (1, 1))
    # equality of both bounds, and a density bound whose product with the SNP count passes 2^63
    p2 = np.array([100, 1100, 2100, 3100], np.int64)
    one = np.array([[0, 0, 3, 0, 0]], np.uint32)                                    # span 3000, 4 SNPs
    for min_bp, dens, want in ((3000, 750, 1), (3001, 750, 0), (3000, 749, 0), (0, 2 ** 62, 1), (3000, 2 ** 63 - 1, 1)):
        keep = np.zeros(1, np.uint8)
        assert lib.gpca_roh_select(vp(one), 1, vp(p2), min_bp, dens, vp(keep)) == _lib.GPCA_OK
        assert int(keep[0]) == want == int(gio.roh_select(one, p2, min_bp, dens)[0]), (min_bp, dens)
    keep = np.zeros(1, np.uint8)
    bad = np.array([[0, 3, 1, 0, 0]], np.uint32)
    assert lib.gpca_roh_select(vp(bad), 1, vp(p2), 0, 5, vp(keep)) == _lib.GPCA_ERR_BAD_ARG
    assert lib.gpca_roh_select(vp(one), -1, vp(p2), 0, 5, vp(keep)) == _lib.GPCA_ERR_BAD_ARG
    assert lib.gpca_roh_select(vp(one), 1, vp(p2), -1, 5, vp(keep)) == _lib.GPCA_ERR_BAD_ARG
    assert lib.gpca_roh_select(vp(one), 1, None, 0, 5, vp(keep)) == _lib.GPCA_ERR_BAD_ARG
    assert lib.gpca_roh_select(None, 0, None, 0, 5, None) == _lib.GPCA_OK
    with pytest.raises(ValueError):
        gio.roh_select(bad, p2, 0, 5)
    assert GpcaEngine.roh_select(np.zeros((0, 5), np.uint32), p2, 0, 5).shape == (0,)


def test_roh_summary_against_its_rule():
    rng = np.random.default_rng(4)
    K, N = 300, 7
    pos = np.cumsum(rng.integers(1, 2000, K)).astype(np.int64)
    brk = np.zeros(K, np.uint8)
    brk[[0, 90, 91, 200]] = 3                                                        # (a domain of one SNP adds no length)
    brk[[40, 150]] = 2
    segs = random_records(rng, K, 80, N)
    keep = (rng.random(80) < 0.6).astype(np.uint8)
    genome = (pos[89] - pos[0]) + 0 + (pos[199] - pos[91]) + (pos[K - 1] - pos[200])
    nseg, total, froh = gio.roh_summary(segs, keep, pos, brk, N)
    for n in range(N):
        mine = [(int(f), int(l)) for (s, f, l, _, _), k in zip(segs, keep) if s == n and k]
        assert nseg[n] == len(mine) and total[n] == sum(int(pos[l]) - int(pos[f]) for f, l in mine)
        assert froh[n] == float(int(total[n])) / float(int(genome))
    assert nseg.dtype == np.int64 and total.dtype == np.int64 and nseg.sum() == keep.sum()
    # no length to divide by: one SNP per chromosome
    _, _, f0 = gio.roh_summary(np.zeros((0, 5), np.uint32), np.zeros(0, np.uint8), pos[:3], np.array([3, 3, 3], np.uint8), 2)
    assert np.isnan(f0).all()


def test_the_bytes_of_hom_and_hom_indiv(tmp_path):
    chroms = ["1"] * 6 + ["2"] * 4
    ids = [f"rs{i}" for i in range(10)]
    pos = np.array([1000, 2500, 4000, 900000, 1200000, 2001000, 500, 1500, 3500, 1000500], np.int64)
    brk = gio.roh_breaks(chroms, pos, 1_000_000)
    assert brk.tolist() == [3, 0, 0, 0, 0, 0, 3, 0, 0, 0]
    segs = np.array([[0, 0, 5, 1, 0], [0, 6, 9, 0, 1], [2, 0, 2, 0, 0], [2, 3, 5, 0, 2]], np.uint32)
    keep = np.array([1, 1, 0, 1], np.uint8)
    pre = str(tmp_path / "o" / "P")
    (tmp_path / "o").mkdir()
    a, b = gio.write_hom(pre, ["f0", "f0", "f1"], ["s0", "s1", "s2"], chroms, ids, pos, segs, keep, brk)
    assert (a, b) == (pre + ".hom", pre + ".hom.indiv")
    assert open(a, "rb").read() == (
        b"#FID\tIID\tCHROM\tSNP1\tSNP2\tPOS1\tPOS2\tKB\tNSNP\tDENSITY\tPHOM\tPHET\n"
        b"f0\ts0\t1\trs0\trs5\t1000\t2001000\t2000\t6\t333.333\t0.833333\t0.166667\n"
        b"f0\ts0\t2\trs6\trs9\t500\t1000500\t1000\t4\t250\t0.75\t0\n"
        b"f1\ts2\t1\trs3\trs5\t900000\t2001000\t1101\t3\t367\t0.333333\t0\n")
    # the genome: (2001000 - 1000) + (1000500 - 500) = 3 000 000 bp
    assert open(b, "rb").read() == (
        b"#FID\tIID\tNSEG\tKB\tKBAVG\tFROH\n"
        b"f0\ts0\t2\t3000\t1500\t1\n"
        b"f0\ts1\t0\t0\tNA\t0\n"
        b"f1\ts2\t1\t1101\t1101\t0.367\n")
    # no length at all: FROH is NA too
    gio.write_hom(pre, ["f0"], ["s0"], ["1", "2"], ["a", "b"], np.array([5, 9], np.int64), np.zeros((0, 5), np.uint32), np.zeros(0, np.uint8),
                  np.array([3, 3], np.uint8))
    assert open(b, "rb").read() == b"#FID\tIID\tNSEG\tKB\tKBAVG\tFROH\nf0\ts0\t0\t0\tNA\tNA\n"
    assert open(a, "rb").read().count(b"\n") == 1


def test_the_threshold_is_the_fraction_of_its_decimal_text():
    t = GpcaEngine.roh_threshold
    assert t(0.05) == (1, 20) and t("0.05") == (1, 20) and t(0.25) == (1, 4) and t(1) == (1, 1) and t(0) == (0, 1) and t(0.1) == (1, 10)
    assert t(0.3) == (3, 10)                                                         # not the double next to 0.3
    from fractions import Fraction
    assert t(Fraction(2, 7)) == (2, 7) and t("3/8") == (3, 8) and t((7, 3)) == (7, 3)   # a pair is passed on as it is
    assert t(1 / 1048576) == (1, 1 << 20)
    for bad in (1e-7, 1 / 3, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError):
            t(bad)
    assert math.isclose(t(0.123456)[0] / t(0.123456)[1], 0.123456) and gpca.GpcaEngine is GpcaEngine
