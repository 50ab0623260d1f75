"""Windowed LD's host side without a GPU: the C ABI entry point, io.ld_windows against a brute-force double loop, io.ld_prune against
a literal restatement of the rule, the id writer, the band split and the flag rules of the Python command line."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from genomic_pca_amd import _lib
from genomic_pca_amd import io as gio
from genomic_pca_amd.cli import main

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ld_window_declared_and_exported(gpca):
    gpca.load()
    hdr = open(os.path.join(ROOT, "include", "gpca.h")).read()
    assert re.search(r"GPCA_API int gpca_ld_window\(gpca_handle\* h, int64_t row0, int64_t row1, const int64_t\* win_end[^,]*, int32_t wmax,\s*"
                     r"double threshold, double\* r2[^,]*, int32_t\* counts[^,]*,\s*uint64_t\* above", hdr)
    assert "#define GPCA_VERSION 250" in hdr
    res, args = _lib.PROTOTYPES["gpca_ld_window"]
    assert res is ctypes.c_int
    assert args[1:] == [ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p,
                        ctypes.c_void_p]
    so = os.path.join(ROOT, "genomic_pca_amd", "libgpca.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T gpca_ld_window$", out, re.M)
    assert "gpca_ld_window(" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = gpca.load()
    assert lib.gpca_ld_window(None, 0, 0, None, 1, 0.0, None, None, None) == _lib.GPCA_ERR_BAD_ARG


def brute_windows(chrom, pos, kind, w):
    K = len(chrom)
    norm = [gio.normalize_chromosome_name(c) for c in chrom]
    out = np.empty(K, np.int64)
    for i in range(K):
        e = i + 1
        while e < K and norm[e] == norm[i] and (e - i < w if kind == "variants" else pos[e] <= pos[i] + w):
            e += 1
        out[i] = e
    return out


def test_ld_windows_against_brute_force():
    rng = np.random.default_rng(1)
    sizes = [1, 37, 400, 2, 150]
    chrom = np.concatenate([[name] * n for name, n in zip(["1", "chr2", "Chr3", "X", "chrchr7"], sizes)])
    pos = np.concatenate([np.sort(rng.integers(1, 400_000, n)) for n in sizes])
    pos[50:55] = pos[50]                                            # ties in position stay inside each other's window
    for text, kind, w in (("50", "variants", 50), ("2", "variants", 2), ("1000", "variants", 1000), ("25kb", "bp", 25_000),
                          ("0.5kb", "bp", 500), ("1000KB", "bp", 1_000_000)):
        assert gio.parse_ld_window(text) == (kind, w)
        we = gio.ld_windows(chrom, pos, text)
        assert we.dtype == np.int64 and np.array_equal(we, brute_windows(chrom, pos, kind, w)), text
        ends = np.cumsum(sizes)
        assert np.all(we[ends - 1] == ends)                         # the last SNP of a chromosome has an empty window
        assert np.all(we > np.arange(len(we))) and np.all(np.diff(we) >= 0)
    assert gio.ld_windows([], [], "50").shape == (0,)
    with pytest.raises(ValueError, match="reappears at variant 3"):
        gio.ld_windows(["1", "1", "2", "chr1"], [1, 2, 3, 4], "50")
    with pytest.raises(ValueError, match="variant 2"):
        gio.ld_windows(["1", "1", "1"], [5, 9, 8], "50")
    gio.ld_windows(["1", "2"], [9, 1], "50")                        # a new chromosome may start lower
    for bad in ("", "abc", "1", "0", "-5", "0kb", "-2kb", "kb", "5mb", "nankb"):
        with pytest.raises(ValueError, match="bad LD window"):
            gio.parse_ld_window(bad)


def pack_above(dense, win_end):
    """dense [K][K] bool (i < j) -> gpca_ld_window's above words for count-free windows win_end"""
    K = dense.shape[0]
    wmax = max(int(np.max(win_end - np.arange(K) - 1)), 1)
    bits = np.zeros((K, (wmax + 63) // 64 * 64), np.uint8)
    for i in range(K):
        n = int(win_end[i]) - i - 1
        bits[i, :n] = dense[i, i + 1:i + 1 + n]
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint64), wmax


def literal_prune(win_end, dense, maf):
    """the rule, word for word"""
    K = len(win_end)
    inn = [True] * K
    for i in range(K):
        if not inn[i]:
            continue
        J = [j for j in range(i + 1, int(win_end[i])) if inn[j] and dense[i, j]]
        jstar = next((j for j in J if maf[j] > maf[i]), None)
        for j in J:
            if jstar is not None and j >= jstar:
                break
            inn[j] = False
        if jstar is not None:
            inn[i] = False
    return np.array(inn, bool)


def test_ld_prune_against_literal_rule():
    rng = np.random.default_rng(2)
    for trial in range(60):
        K = int(rng.integers(1, 120))
        w = int(rng.integers(2, 80))
        win_end = np.minimum(np.arange(K) + w, K).astype(np.int64)
        if trial % 3 == 0 and K > 10:                               # a chromosome boundary
            win_end[:K // 2] = np.minimum(win_end[:K // 2], K // 2)
        dense = np.triu(rng.random((K, K)) < rng.choice([0.02, 0.2, 0.7]), 1)
        maf = rng.integers(1, 6, K) / 10.0                          # many ties
        above, wmax = pack_above(dense, win_end)
        want = literal_prune(win_end, dense, maf)
        got = gio.ld_prune(win_end, above, maf)
        assert got.dtype == bool and np.array_equal(got, want), trial
        cuts = sorted({0, K} | set(rng.integers(0, K + 1, 3).tolist()))
        banded = gio.ld_prune(win_end, (((a, b), above[a:b]) for a, b in zip(cuts[:-1], cuts[1:])), maf)
        assert np.array_equal(banded, want), trial
        # the survivor invariant: no two survivors within a window are above the threshold
        for i in np.flatnonzero(got):
            assert not any(got[j] and dense[i, j] for j in range(i + 1, int(win_end[i])))
    # of a pair the smaller MAF leaves, ties the later one; once i has left its window is not looked at further
    we = np.array([3, 3, 3], np.int64)
    d = np.zeros((3, 3), bool); d[0, 1] = d[0, 2] = True
    assert gio.ld_prune(we, pack_above(d, we)[0], np.array([0.3, 0.1, 0.2])).tolist() == [True, False, False]
    assert gio.ld_prune(we, pack_above(d, we)[0], np.array([0.2, 0.2, 0.2])).tolist() == [True, False, False]
    assert gio.ld_prune(we, pack_above(d, we)[0], np.array([0.2, 0.1, 0.3])).tolist() == [False, False, True]
    assert gio.ld_prune(we, pack_above(d, we)[0], np.array([0.1, 0.3, 0.05])).tolist() == [False, True, True]
    with pytest.raises(ValueError):
        gio.ld_prune(we, [((0, 2), np.zeros((2, 1), np.uint64))], np.zeros(3))
    with pytest.raises(ValueError):
        gio.ld_prune(we, np.zeros((3, 1), np.uint64), np.zeros(2))


def test_maf_and_bands():
    maf = gio.maf_from_qc_detail([10, 10, 0, 4], [2, 0, 0, 0], [1, 10, 0, 4])
    assert maf.tolist() == [0.2, 0.0, 0.0, 0.0] and maf.dtype == np.float64
    rng = np.random.default_rng(3)
    K = 500
    we = np.minimum(np.arange(K) + 1 + rng.integers(0, 90, K), K)
    we = np.maximum.accumulate(we)
    for cap in (1, 64, 5000, 1 << 26):
        bands = list(gio.ld_bands(we, cap))
        assert bands[0][0] == 0 and bands[-1][1] == K and all(a[1] == b[0] for a, b in zip(bands, bands[1:]))
        for r0, r1, wm in bands:
            assert wm == max(int(np.max(we[r0:r1] - np.arange(r0, r1) - 1)), 1)
            assert r1 - r0 == 1 or (r1 - r0) * wm <= cap
    assert list(gio.ld_bands(np.zeros(0, np.int64))) == []


def test_write_prune_ids(tmp_path):
    pre = str(tmp_path / "o")
    paths = gio.write_prune_ids(pre, ["rs1", "rs2", "rs3", "rs4"], np.array([True, False, False, True]))
    assert paths == (pre + ".prune.in", pre + ".prune.out")
    assert open(paths[0]).read() == "rs1\nrs4\n" and open(paths[1]).read() == "rs2\nrs3\n"
    with pytest.raises(ValueError):
        gio.write_prune_ids(pre, ["a"], np.array([True, False]))


BASE = ["--bed-file", "t.bed", "--ld-block-file", "l.txt", "--out", "x"]
BAD_FLAGS = [
    (["--gpca-indep-pairwise", "50", "0.2"], "--gpca-indep-pairwise needs the --eigensnp workflow"),
    (["--eigensnp", "--gpca-indep-pairwise", "50", "0"], "--gpca-indep-pairwise R2 must lie in (0, 1)"),
    (["--eigensnp", "--gpca-indep-pairwise", "50", "1"], "--gpca-indep-pairwise R2 must lie in (0, 1)"),
    (["--eigensnp", "--gpca-indep-pairwise", "50", "nan"], "--gpca-indep-pairwise R2 must lie in (0, 1)"),
    (["--eigensnp", "--gpca-indep-pairwise", "50", "x"], "--gpca-indep-pairwise R2 must lie in (0, 1)"),
    (["--eigensnp", "--gpca-indep-pairwise", "fifty", "0.2"], "bad LD window 'fifty'"),
    (["--eigensnp", "--gpca-indep-pairwise", "1", "0.2"], "bad LD window '1'"),
    (["--eigensnp", "--gpca-indep-pairwise", "0kb", "0.2"], "bad LD window '0kb'"),
]


@pytest.mark.parametrize("flags,msg", BAD_FLAGS)
def test_flag_errors_python(flags, msg):
    with pytest.raises(SystemExit) as ei:
        main(BASE + flags)
    assert msg in str(ei.value)
