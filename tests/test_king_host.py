"""KING's host side without a GPU: the greedy pruning rule (io.king_unrelated and the C++ twin in formats.hpp), the .kin0 layout and
its filter, the band split of the strict triangle, the flag rules of both command lines, and the C ABI entry point."""
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
BIN = os.path.join(ROOT, "genomic_pca_amd", "bin", "genomic_pca")


def out_set(n, pairs):
    return [int(i) for i in np.flatnonzero(~gio.king_unrelated(n, pairs))]


def test_greedy_rule():
    assert out_set(4, []) == []
    assert out_set(2, [(0, 1)]) == [1]                             # a tie goes to the later sample
    assert out_set(2, [(1, 0)]) == [1]
    assert out_set(5, [(0, 1), (1, 2), (2, 3)]) == [1, 2]          # chain 0-1-2-3: 1 and 2 tie at two partners -> 2, then 0-1 -> 1
    assert out_set(5, [(0, 1), (1, 2)]) == [1]                     # the middle of a chain of three
    assert out_set(4, [(0, 1), (1, 2), (0, 2)]) == [1, 2]          # triangle: all tie -> 2, then 0-1 -> 1
    assert out_set(6, [(0, 5), (1, 5), (2, 5), (3, 4)]) == [4, 5]  # the hub first
    assert out_set(3, [(0, 1), (0, 1)]) == [1]                     # a pair listed twice counts once
    kin = np.array([0.3, np.nan, 0.01])                            # NaN never counts: the caller keeps only kinship > cutoff
    j, k = gio.band_pairs(0, 3)
    hit = np.flatnonzero(kin > 0.0884)
    assert out_set(3, list(zip(k[hit], j[hit]))) == [1]
    with pytest.raises(ValueError):
        gio.king_unrelated(3, [(0, 3)])


def test_band_pairs_and_bands():
    j, k = gio.band_pairs(0, 4)
    assert list(zip(j, k)) == [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)]
    j, k = gio.band_pairs(3, 5)
    assert list(zip(j, k)) == [(3, 0), (3, 1), (3, 2), (4, 0), (4, 1), (4, 2), (4, 3)]
    for n, cap in ((1, 4), (10, 4), (100, 1000), (37, 1)):
        bands = list(gio.king_bands(n, cap))
        assert bands[0][0] == 0 and bands[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(bands, bands[1:]))
        assert all(r1 - r0 == 1 or r1 * (r1 - 1) // 2 - r0 * (r0 - 1) // 2 <= cap for r0, r1 in bands)


def test_write_kin0_layout_and_filter(tmp_path):
    n = 4
    fids, iids = [f"F{i}" for i in range(n)], [f"I{i}" for i in range(n)]
    kin = np.array([0.5, -0.0123456789, np.nan, 0.25, 0.0884, 0.08839999])
    cnt = np.arange(18, dtype=np.int32).reshape(6, 3)
    bands = [((0, 1), kin[:0], cnt[:0]), ((1, 3), kin[:3], cnt[:3]), ((3, 4), kin[3:], cnt[3:])]
    pre = str(tmp_path / "o")
    path = gio.write_kin0(pre, fids, iids, iter(bands))
    assert path == pre + ".kin0"
    lines = open(path).read().split("\n")
    assert lines[0] == "#FID1\tIID1\tFID2\tIID2\tNSNP\tHETHET\tIBS0\tKINSHIP" and lines[-1] == ""
    assert lines[1:-1] == ["F0\tI0\tF1\tI1\t0\t1\t2\t0.500000", "F0\tI0\tF2\tI2\t3\t4\t5\t-0.012346", "F1\tI1\tF2\tI2\t6\t7\t8\tnan",
                           "F0\tI0\tF3\tI3\t9\t10\t11\t0.250000", "F1\tI1\tF3\tI3\t12\t13\t14\t0.088400",
                           "F2\tI2\tF3\tI3\t15\t16\t17\t0.088400"]
    gio.write_kin0(pre, fids, iids, iter(bands), min_kinship=0.0884)
    got = open(path).read().split("\n")[1:-1]
    assert [ln.split("\t")[3] for ln in got] == ["I1", "I3", "I3"]           # 0.5, 0.25, 0.0884 (not NaN, not 0.08839999)
    with pytest.raises(ValueError):
        gio.write_kin0(pre, fids, iids, iter(bands[:2]))
    with pytest.raises(ValueError):
        gio.write_kin0(pre, fids, iids, iter([bands[0], bands[2]]))


def test_write_king_cutoff_ids(tmp_path):
    pre = str(tmp_path / "o")
    paths = gio.write_king_cutoff_ids(pre, ["a", "b", "c"], ["x", "y", "z"], np.array([True, False, True]))
    assert paths == (pre + ".king.cutoff.in.id", pre + ".king.cutoff.out.id")
    assert open(paths[0]).read() == "#FID\tIID\na\tx\nc\tz\n"
    assert open(paths[1]).read() == "#FID\tIID\nb\ty\n"


def test_cpp_greedy_rule_and_kin0_match_python(tmp_path):
    """formats.hpp's king_unrelated and Kin0Writer against io.py on random graphs and a filtered table"""
    src = tmp_path / "drv.cpp"
    src.write_text(r'''
#include "formats.hpp"
#include <iostream>
int main() {
    int64_t n, m;
    while (std::cin >> n >> m) {
        std::vector<std::pair<int64_t, int64_t>> p((size_t)m);
        for (auto& q : p) std::cin >> q.first >> q.second;
        for (uint8_t v : gpca_host::king_unrelated(n, p)) std::cout << int(v);
        std::cout << "\n";
    }
    std::vector<std::string> f = {"F0", "F1", "F2", "F3"}, i = {"I0", "I1", "I2", "I3"};
    gpca_host::Kin0Writer w(std::string(std::getenv("KIN0_PREFIX")), f, i, true, 0.0884);
    const double k1[3] = {0.5, -0.0123456789, 0.0 / 0.0}, k2[3] = {0.25, 0.0884, 0.08839999};
    int32_t c[18];
    for (int t = 0; t < 18; ++t) c[t] = t;
    w.add_band(0, 1, nullptr, nullptr); w.add_band(1, 3, k1, c); w.add_band(3, 4, k2, c + 9); w.close();
    return 0;
}
''')
    exe = str(tmp_path / "drv")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "genomic_pca_amd", "host"), str(src), "-lz", "-o", exe])
    rng = np.random.default_rng(3)
    cases, want = [], []
    for _ in range(200):
        n = int(rng.integers(2, 30))
        m = int(rng.integers(0, 3 * n))
        pairs = [tuple(sorted(rng.choice(n, 2, replace=False).tolist())) for _ in range(m)]
        cases.append(f"{n} {m} " + " ".join(f"{a} {b}" for a, b in pairs))
        want.append("".join(str(int(v)) for v in gio.king_unrelated(n, pairs)))
    env = dict(os.environ, KIN0_PREFIX=str(tmp_path / "c"))
    out = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, env=env, check=True).stdout.split()
    assert out == want
    kin = np.array([0.5, -0.0123456789, np.nan, 0.25, 0.0884, 0.08839999])
    cnt = np.arange(18, dtype=np.int32).reshape(6, 3)
    bands = [((0, 1), kin[:0], cnt[:0]), ((1, 3), kin[:3], cnt[:3]), ((3, 4), kin[3:], cnt[3:])]
    gio.write_kin0(str(tmp_path / "p"), ["F0", "F1", "F2", "F3"], ["I0", "I1", "I2", "I3"], iter(bands), min_kinship=0.0884)
    assert open(str(tmp_path / "c.kin0"), "rb").read() == open(str(tmp_path / "p.kin0"), "rb").read()


BASE = ["--bed-file", "t.bed", "--ld-block-file", "l.txt", "--out", "x"]
BAD_FLAGS = [
    (["--gpca-make-king"], "need the --eigensnp workflow"),
    (["--gpca-king-cutoff", "0.1"], "need the --eigensnp workflow"),
    (["--eigensnp", "--gpca-king-table-filter", "0.1"], "--gpca-king-table-filter needs --gpca-make-king"),
    (["--eigensnp", "--gpca-king-cutoff", "0.5"], "--gpca-king-cutoff must lie in (0, 0.5)"),
    (["--eigensnp", "--gpca-king-cutoff", "0"], "--gpca-king-cutoff must lie in (0, 0.5)"),
    (["--eigensnp", "--gpca-king-cutoff", "nan"], "--gpca-king-cutoff must lie in (0, 0.5)"),
    (["--eigensnp", "--gpca-king-cutoff", "0.0884", "--gpca-eigensnp-local-stage"], "cannot be combined with --gpca-eigensnp-local-stage"),
]


@pytest.mark.parametrize("flags,msg", BAD_FLAGS)
def test_flag_errors_python(flags, msg):
    with pytest.raises(SystemExit) as ei:
        main(BASE + flags)
    assert msg in str(ei.value)


@pytest.fixture(scope="module")
def host_bin(gpca):
    gpca.load()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "genomic_pca_amd", "host"), "-s"])
    return BIN


@pytest.mark.parametrize("flags,msg", BAD_FLAGS)
def test_flag_errors_cpp(host_bin, flags, msg):
    r = subprocess.run([host_bin, *BASE, *flags], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and msg in r.stderr, r.stderr
    h = subprocess.run([host_bin, "--help"], capture_output=True, text=True, timeout=60).stdout
    for f in ("--gpca-make-king", "--gpca-king-table-filter", "--gpca-king-cutoff"):
        assert f in h


def test_king_declared_and_exported(gpca):
    gpca.load()                                                   # (builds libgpca.so when it is missing)
    hdr = open(os.path.join(ROOT, "include", "gpca.h")).read()
    assert re.search(r"GPCA_API int gpca_king\(gpca_handle\* h, int64_t row0, int64_t row1, double\* kinship, int32_t\* counts", hdr)
    res, args = _lib.PROTOTYPES["gpca_king"]
    assert res is ctypes.c_int and args[1:] == [ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    so = os.path.join(ROOT, "genomic_pca_amd", "libgpca.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T gpca_king$", out, re.M)
    assert "gpca_king(" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
