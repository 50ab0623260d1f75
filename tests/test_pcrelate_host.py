"""CPU-only: the host side of PC-Relate: the files io.write_pcrelate writes (formatting, the table filter, nan), its bands, the C++
twin of the writer (formats.hpp, byte for byte), and the flag rules and refusals of both command lines."""
import os
import subprocess

import numpy as np
import pytest

from genomic_pca_amd import io
from genomic_pca_amd.cli import main

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tri(n):
    kin = np.zeros((n, n))
    cnt = np.zeros((n, n), np.int32)
    for a in range(n):
        for b in range(a + 1):
            kin[a, b] = 0.5 + 0.01 * a if a == b else 0.001 * (a * 10 + b) - 0.01
            cnt[a, b] = 1000 + 10 * a + b
    return kin, cnt


def _band(kin, cnt, r0, r1):
    il = [(a, b) for a in range(r0, r1) for b in range(a + 1)]
    return (r0, r1), np.array([kin[a, b] for a, b in il]), np.array([cnt[a, b] for a, b in il], np.int32)


def test_write_pcrelate_formats_filters_and_nan(tmp_path):
    n = 5
    kin, cnt = _tri(n)
    kin[3, 1] = np.nan
    kin[4, 4] = np.nan
    fids, iids = [f"F{i}" for i in range(n)], [f"I{i}" for i in range(n)]
    bands = [_band(kin, cnt, 0, 2), _band(kin, cnt, 2, 3), _band(kin, cnt, 3, 5)]
    pk, pi = io.write_pcrelate(str(tmp_path / "out"), fids, iids, bands)
    assert pk.endswith("out.pcrelate.kin") and pi.endswith("out.pcrelate.inbreed")
    lines = open(pk).read().split("\n")
    assert lines[0] == "#FID1\tIID1\tFID2\tIID2\tNSNP\tKINSHIP" and lines[-1] == ""
    rows = [l.split("\t") for l in lines[1:-1]]
    assert len(rows) == n * (n - 1) // 2
    assert rows[0] == ["F0", "I0", "F1", "I1", "1010", "0.000000"]                 # pair (1, 0): ID1 the earlier sample
    assert rows[1] == ["F0", "I0", "F2", "I2", "1020", "0.010000"]
    assert ["F1", "I1", "F3", "I3", "1031", "nan"] in rows
    assert rows[-1] == ["F3", "I3", "F4", "I4", "1043", f"{kin[4, 3]:.6f}"]
    inb = open(pi).read().split("\n")
    assert inb[0] == "#FID\tIID\tNSNP\tF" and len(inb) == n + 2
    assert inb[1] == "F0\tI0\t1000\t0.000000" and inb[3] == "F2\tI2\t1022\t0.040000" and inb[5] == "F4\tI4\t1044\tnan"
    # the table filter: only pairs at or above it, NaN never passes; the inbreeding file is whole
    io.write_pcrelate(str(tmp_path / "f"), fids, iids, [_band(kin, cnt, 0, n)], min_kinship=0.02)
    kept = [l.split("\t") for l in open(str(tmp_path / "f.pcrelate.kin")).read().split("\n")[1:-1]]
    want = [(a, b) for a in range(n) for b in range(a) if kin[a, b] >= 0.02]
    assert [(r[3], r[1]) for r in kept] == [(f"I{a}", f"I{b}") for a, b in want] and 0 < len(want) < n * (n - 1) // 2
    assert open(str(tmp_path / "f.pcrelate.inbreed")).read() == open(pi).read()


def test_write_pcrelate_refuses_bad_bands(tmp_path):
    kin, cnt = _tri(4)
    ids = ["a", "b", "c", "d"]
    with pytest.raises(ValueError):
        io.write_pcrelate(str(tmp_path / "x"), ids, ids, [_band(kin, cnt, 1, 4)])              # does not start at row 0
    with pytest.raises(ValueError):
        io.write_pcrelate(str(tmp_path / "x"), ids, ids, [_band(kin, cnt, 0, 3)])              # ends early
    with pytest.raises(ValueError):
        io.write_pcrelate(str(tmp_path / "x"), ids, ids, [((0, 4), np.zeros(9), np.zeros(9))])    # wrong size
    with pytest.raises(ValueError):
        io.write_pcrelate(str(tmp_path / "x"), ids[:3], ids, [_band(kin, cnt, 0, 4)])


def test_pcrelate_bands_cover_the_triangle():
    for n, cap in ((1, 1), (7, 5), (100, 333), (1000, 1 << 26)):
        bands = list(io.pcrelate_bands(n, cap))
        assert bands[0][0] == 0 and bands[-1][1] == n and all(a[1] == b[0] for a, b in zip(bands, bands[1:]))
        for r0, r1 in bands:
            assert r1 > r0 and (r1 == r0 + 1 or r1 * (r1 + 1) // 2 - r0 * (r0 + 1) // 2 <= cap)


def test_cpp_writer_matches_python(tmp_path):
    """formats.hpp's PcrelateWriter against io.write_pcrelate on a banded, filtered table with NaNs"""
    n = 5
    kin, cnt = _tri(n)
    kin[3, 1] = np.nan
    kin[4, 4] = np.nan
    kin[2, 0] = -0.0123456789
    bands = [_band(kin, cnt, 0, 1), _band(kin, cnt, 1, 4), _band(kin, cnt, 4, 5)]
    arr = lambda v, f: ", ".join("0.0 / 0.0" if x != x else f(x) for x in v)
    calls = "".join(f"{{ const double k[] = {{{arr(k, lambda x: repr(float(x)))}}}; const int32_t c[] = {{{arr(c, str)}}}; w.add_band({r0}, {r1}, k, c); }}\n"
                    for (r0, r1), k, c in bands)
    src = tmp_path / "drv.cpp"
    src.write_text('''
#include "formats.hpp"
int main(int argc, char** argv) {
    std::vector<std::string> f = {"F0", "F1", "F2", "F3", "F4"}, i = {"I0", "I1", "I2", "I3", "I4"};
    for (int filt = 0; filt < 2; ++filt) {
        gpca_host::PcrelateWriter w(std::string(argv[1]) + (filt ? "f" : "a"), f, i, filt != 0, 0.02);
        ''' + calls + '''
        w.close();
    }
    gpca_host::PcrelateWriter bad(std::string(argv[1]) + "x", f, i, false, 0.0);
    try { bad.add_band(1, 2, nullptr, nullptr); return 1; } catch (const std::runtime_error&) {}
    try { bad.close(); return 1; } catch (const std::runtime_error&) {}
    return 0;
}
''')
    exe = str(tmp_path / "drv")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "genomic_pca_amd", "host"), str(src), "-lz", "-o", exe])
    subprocess.run([exe, str(tmp_path / "c")], check=True, timeout=60)
    fids, iids = [f"F{i}" for i in range(n)], [f"I{i}" for i in range(n)]
    io.write_pcrelate(str(tmp_path / "pa"), fids, iids, bands)
    io.write_pcrelate(str(tmp_path / "pf"), fids, iids, bands, min_kinship=0.02)
    for t in "af":
        for ext in (".pcrelate.kin", ".pcrelate.inbreed"):
            assert open(str(tmp_path / ("c" + t)) + ext, "rb").read() == open(str(tmp_path / ("p" + t)) + ext, "rb").read(), (t, ext)
    assert open(str(tmp_path / "cf.pcrelate.kin")).read().count("\n") < open(str(tmp_path / "ca.pcrelate.kin")).read().count("\n")


BASE = ["--bed-file", "t.bed", "--ld-block-file", "l.txt", "--out", "x"]
RESIDENT = "--gpca-make-pcrelate needs the genotype matrix resident on the device"
BAD_FLAGS = [
    (["--gpca-make-pcrelate", "2"], "--gpca-make-pcrelate needs the --eigensnp workflow"),
    (["--eigensnp", "--gpca-pcrelate-maf-bound", "0.02"], "need --gpca-make-pcrelate"),
    (["--eigensnp", "--gpca-pcrelate-table-filter", "0.1"], "need --gpca-make-pcrelate"),
    (["--eigensnp", "--gpca-make-pcrelate", "-1"], "--gpca-make-pcrelate P must lie in [0, min(--eigensnp-k-global, 32)]"),
    (["--eigensnp", "--gpca-make-pcrelate", "11"], "--gpca-make-pcrelate P must lie in [0, min(--eigensnp-k-global, 32)]"),
    (["--eigensnp", "--eigensnp-k-global", "3", "--gpca-make-pcrelate", "4"], "--gpca-make-pcrelate P must lie in"),
    (["--eigensnp", "--eigensnp-k-global", "40", "--gpca-make-pcrelate", "33"], "--gpca-make-pcrelate P must lie in"),
    (["--eigensnp", "--gpca-make-pcrelate", "2", "--gpca-pcrelate-maf-bound", "0.5"], "--gpca-pcrelate-maf-bound must lie in [0, 0.5)"),
    (["--eigensnp", "--gpca-make-pcrelate", "2", "--gpca-pcrelate-maf-bound", "-0.1"], "--gpca-pcrelate-maf-bound must lie in [0, 0.5)"),
    (["--eigensnp", "--gpca-make-pcrelate", "2", "--gpca-pcrelate-maf-bound", "nan"], "--gpca-pcrelate-maf-bound must lie in [0, 0.5)"),
    (["--eigensnp", "--gpca-make-pcrelate", "2", "--gpca-eigensnp-local-stage"], "cannot be combined with --gpca-eigensnp-local-stage"),
    (["--eigensnp", "--gpca-make-pcrelate", "0", "--gpca-stream", "on"], RESIDENT),
]


@pytest.mark.parametrize("flags,msg", BAD_FLAGS)
def test_flag_errors_python(flags, msg):
    with pytest.raises(SystemExit) as ei:
        main(BASE + flags)
    assert msg in str(ei.value)


def test_flags_parse_python():
    from genomic_pca_amd.cli import build_parser
    a = build_parser().parse_args(BASE + ["--eigensnp", "--gpca-make-pcrelate", "0"])
    assert a.gpca_make_pcrelate == 0 and a.gpca_pcrelate_maf_bound is None and a.gpca_pcrelate_table_filter is None
    a = build_parser().parse_args(BASE + ["--gpca-make-pcrelate=3", "--gpca-pcrelate-maf-bound", "0.05", "--gpca-pcrelate-table-filter", "-0.1"])
    assert a.gpca_make_pcrelate == 3 and a.gpca_pcrelate_maf_bound == 0.05 and a.gpca_pcrelate_table_filter == -0.1
    assert build_parser().parse_args(BASE).gpca_make_pcrelate is None


@pytest.fixture(scope="module")
def host_bin(gpca):
    gpca.load()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "genomic_pca_amd", "host"), "-s"])
    return os.path.join(ROOT, "genomic_pca_amd", "bin", "genomic_pca")


@pytest.mark.parametrize("flags,msg", BAD_FLAGS)
def test_flag_errors_cpp(host_bin, flags, msg):
    r = subprocess.run([host_bin, *BASE, *flags], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and msg in r.stderr, r.stderr


def test_flags_parse_cpp(host_bin):
    h = subprocess.run([host_bin, "--help"], capture_output=True, text=True, timeout=60).stdout
    for f in ("--gpca-make-pcrelate", "--gpca-pcrelate-maf-bound", "--gpca-pcrelate-table-filter"):
        assert f in h
    # a value that is no number, and a flag without its value, are usage errors
    for bad in (["--gpca-make-pcrelate", "two"], ["--gpca-pcrelate-maf-bound", "x"], ["--gpca-make-pcrelate"]):
        r = subprocess.run([host_bin, *BASE, "--eigensnp", *bad], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--gpca-" in r.stderr, r.stderr
