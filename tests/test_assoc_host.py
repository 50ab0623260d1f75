"""CPU-only: the host pieces of the association scan -- gpca_student_t_log10p (gpca_assoc.cpp), the phenotype reader, the alignment
to .fam order, the bands and the writer of genomic_pca_amd/io.py with their twins in host/formats.hpp, and the rules of the
--gpca-assoc-* flags of cli.py.

gpca_student_t_log10p against mpmath at 50 digits (-log10 of the regularised incomplete beta function I_x(df / 2, 1 / 2), x = df / (df +
t^2), as ln 2 + ln f(t) + ln of the integral of f(s) / f(t) over s >= t by quadrature) on the grid df in {1, 2, 5, 30, 1e3, 5e5} x |t| in {0, 1e-3, 1, 5, 40, 200}; the grid reaches -log10 p = 8 358 (df = 5e5, t = 200),
far past the 308 where p itself underflows.  Largest relative error measured on the grid: 1.8e-13 (df = 5e5, t = 5); the bar is 8 times
that, 1.5e-12, well inside the 1e-9 that six printed digits need.  scipy.stats.t.sf is cross-checked where 2 sf does not underflow."""
import math
import os
import subprocess

import numpy as np
import pytest

from genomic_pca_amd import _lib, io as gio
from genomic_pca_amd.cli import main

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = 1.8e-13
BAR = 8 * WORST
assert BAR <= 1e-9
DFS = [1, 2, 5, 30, 1e3, 5e5]
TS = [0, 1e-3, 1, 5, 40, 200]


def test_student_t_log10p_against_mpmath():
    import mpmath as mp
    from scipy import stats
    f = _lib.load().gpca_student_t_log10p
    worst, top = 0.0, 0.0
    with mp.workdps(50):
        for df in DFS:
            for t in TS:
                got = f(float(t), float(df))
                assert got == f(-float(t), float(df))
                if t == 0:
                    assert got == 0.0
                    continue
                ref = _mp_log10p(mp, t, df)
                rel = float(abs((mp.mpf(got) - ref) / ref))
                worst, top = max(worst, rel), max(top, float(ref))
                assert rel <= BAR, (df, t, got, float(ref), rel)
                p2 = 2 * stats.t.sf(float(t), float(df))
                if p2 > 1e-300:
                    assert abs(got + math.log10(p2)) <= 1e-9 * max(got, 1e-3) + 1e-12, (df, t, got, p2)
    print("largest relative error on the grid", worst, "largest -log10 p", top)
    assert top > 308
    assert math.isnan(f(float("nan"), 5.0)) and math.isnan(f(1.0, 0.0)) and f(float("inf"), 5.0) == float("inf")


def _mp_log10p(mp, t, df):
    """-log10(2 int_t^inf f), f the t density: ln f(t) in logarithms, the integral of f(s) / f(t) by quadrature (no underflow)"""
    t, nu = mp.mpf(t), mp.mpf(df)
    ln_f = mp.loggamma((nu + 1) / 2) - mp.loggamma(nu / 2) - mp.log(nu * mp.pi) / 2 - (nu + 1) / 2 * mp.log1p(t * t / nu)
    ratio = lambda s: mp.exp(-(nu + 1) / 2 * (mp.log1p(s * s / nu) - mp.log1p(t * t / nu)))
    w = 1 / (t * (nu + 1) / (nu + t * t))                # the e-folding length of the tail at t
    cuts = [t] + [t + w * k for k in (1, 4, 16, 64, 256)] + [mp.inf]
    return -(mp.log(2) + ln_f + mp.log(mp.quad(ratio, cuts))) / mp.log(10)


def _write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return str(path)


def test_read_and_align_pheno(tmp_path):
    p = _write(tmp_path / "a.pheno", "FID IID height bmi\nf2 s2 1.5 NA\nf0 s0 -2 3e1\n\nf9 s9 7 8\nf1 s1 nan 0.25\n")
    tab = gio.read_pheno(p)
    assert tab.names == ["height", "bmi"] and tab.sample_ids == ["s2", "s0", "s9", "s1"] and tab.values.shape == (4, 2)
    got = gio.align_pheno(tab, ["f0", "f1", "f2", "f3"], ["s0", "s1", "s2", "s3"])
    want = np.array([[-2, 30], [np.nan, 0.25], [1.5, np.nan], [np.nan, np.nan]])
    assert np.array_equal(got, want, equal_nan=True)
    # the same IID under another FID is another sample
    assert np.isnan(gio.align_pheno(tab, ["fx"], ["s0"])).all()
    assert gio.read_pheno(_write(tmp_path / "h.pheno", "#FID\tIID\ty\nf s 1\n")).names == ["y"]
    with pytest.raises(ValueError, match="appears twice"):
        gio.read_pheno(_write(tmp_path / "d.pheno", "FID IID y\nf0 s0 1\nf1 s1 2\nf0 s0 3\n"))
    with pytest.raises(ValueError, match="header"):
        gio.read_pheno(_write(tmp_path / "n.pheno", "f0 s0 1\nf1 s1 2\n"))
    with pytest.raises(ValueError, match="header"):
        gio.read_pheno(_write(tmp_path / "e.pheno", "FID IID\nf0 s0\n"))
    with pytest.raises(ValueError, match="fields"):
        gio.read_pheno(_write(tmp_path / "s.pheno", "FID IID y\nf0 s0 1 2\n"))
    with pytest.raises(ValueError, match="not a number"):
        gio.read_pheno(_write(tmp_path / "x.pheno", "FID IID y\nf0 s0 tall\n"))


def test_assoc_bands():
    assert gio.assoc_bands(0, 5) == []
    assert gio.assoc_bands(10, 64, max_values=64 * 4) == [(0, 4), (4, 8), (8, 10)]
    assert gio.assoc_bands(3, 64, max_values=1) == [(0, 1), (1, 2), (2, 3)]
    assert gio.assoc_bands(1000, 33) == [(0, 1000)]


def test_write_assoc_against_a_literal_file(tmp_path):
    prefix = str(tmp_path / "out" / "run")
    nan = float("nan")
    path = gio.write_assoc(prefix, "height", ["1", "1", "X"], [100, 2500000, 7], ["rs1", "rs2", "rs3"], ["A", "G", "T"],
                           [500.0, 499.0, 0.0], [0.25, 0.123456789, nan], [1.5, -2.5e-7, nan], [0.5, 1e-7, nan], [3.0, -2.5, nan],
                           [2.56789012, 1234.5678, nan])
    assert path == prefix + ".height.assoc.linear"
    gio.write_assoc(prefix, "height", ["2"], [9], ["rs4"], ["C"], [12.0], [0.5], [1e10], [123456789.0], [0.0], [0.0], append=True)
    want = ("#CHROM\tPOS\tID\tA1\tOBS_CT\tA1_FREQ\tBETA\tSE\tT_STAT\tLOG10P\n"
            "1\t100\trs1\tA\t500\t0.25\t1.5\t0.5\t3\t2.56789\n"
            "1\t2500000\trs2\tG\t499\t0.123457\t-2.5e-07\t1e-07\t-2.5\t1234.57\n"
            "X\t7\trs3\tT\t0\tNA\tNA\tNA\tNA\tNA\n"
            "2\t9\trs4\tC\t12\t0.5\t1e+10\t1.23457e+08\t0\t0\n")
    assert open(path).read() == want
    with pytest.raises(ValueError):
        gio.write_assoc(prefix, "bmi", ["1"], [1, 2], ["a"], ["A"], [1], [1], [1], [1], [1], [1])


# ------------------------------------------------------------------------------------------------ the flags of both command lines
BASE = ["--bed-file", "t.bed", "--ld-block-file", "l.txt", "--out", "x"]
NEEDS_RESIDENT = "--gpca-assoc-pheno needs the genotype matrix resident on the device"


def pheno_files(d):
    """{name: path}: a good table of 2 traits, one of 60 traits, a covariate table of 3 columns, and the refused ones"""
    ids = [f"f{i} s{i}" for i in range(6)]
    return {
        "ok": _write(d / "ok.pheno", "FID IID t1 t2\n" + "".join(f"{s} {i} {i * i}\n" for i, s in enumerate(ids))),
        "wide": _write(d / "wide.pheno", "FID IID " + " ".join(f"y{j}" for j in range(60)) + "\n" + "".join(s + " 1" * 60 + "\n" for s in ids)),
        "cov": _write(d / "cov.txt", "FID IID age sex batch\n" + "".join(f"{s} 4{i} {i % 2} {i % 3}\n" for i, s in enumerate(ids))),
        "dup": _write(d / "dup.pheno", "FID IID y\nf0 s0 1\nf0 s0 2\n"),
        "nohead": _write(d / "nohead.pheno", "f0 s0 1\n"),
        "word": _write(d / "word.pheno", "FID IID y\nf0 s0 1_0\n"),
        "absent": str(d / "absent.pheno"),
    }


def bad_flags(f):
    """(flags, message) for every refusal of the --gpca-assoc-* flags that needs no device"""
    E = ["--eigensnp", "--gpca-assoc-pheno", f["ok"]]
    return [
        (["--gpca-assoc-pheno", f["ok"]], "--gpca-assoc-pheno needs the --eigensnp workflow"),
        (["--eigensnp", "--gpca-assoc-pcs", "2"], "--gpca-assoc-pcs, --gpca-assoc-covar and --gpca-assoc-vif need --gpca-assoc-pheno"),
        (["--eigensnp", "--gpca-assoc-covar", f["cov"]], "need --gpca-assoc-pheno"),
        (["--eigensnp", "--gpca-assoc-vif", "10"], "need --gpca-assoc-pheno"),
        (E + ["--gpca-assoc-pcs", "-1"], "--gpca-assoc-pcs P must lie in [0, --eigensnp-k-global]"),
        (E + ["--gpca-assoc-pcs", "11"], "--gpca-assoc-pcs P must lie in [0, --eigensnp-k-global]"),
        (E + ["--eigensnp-k-global", "4", "--gpca-assoc-pcs", "5"], "--gpca-assoc-pcs P must lie in [0, --eigensnp-k-global]"),
        (E + ["--gpca-assoc-vif", "0.5"], "--gpca-assoc-vif must be finite and at least 1"),
        (E + ["--gpca-assoc-vif", "inf"], "--gpca-assoc-vif must be finite and at least 1"),
        (E + ["--gpca-assoc-vif", "nan"], "--gpca-assoc-vif must be finite and at least 1"),
        (E + ["--gpca-eigensnp-local-stage"], "--gpca-assoc-pheno cannot be combined with --gpca-eigensnp-local-stage (that stage defines no all-sample scores)"),
        (E + ["--gpca-stream", "on"], NEEDS_RESIDENT),
        # T + Pc > 64: 60 traits + 10 PCs (the default, k-global); 60 + 2 + 3; 2 + 62 PCs + 3; and 60 + 4 + 0 = 64 is fine (below)
        (["--eigensnp", "--gpca-assoc-pheno", f["wide"]], "60 traits + 10 PCs + 0 covariates are more than 64 columns"),
        (["--eigensnp", "--gpca-assoc-pheno", f["wide"], "--gpca-assoc-pcs", "2", "--gpca-assoc-covar", f["cov"]],
         "60 traits + 2 PCs + 3 covariates are more than 64 columns"),
        (E + ["--eigensnp-k-global", "62", "--gpca-assoc-covar", f["cov"]], "2 traits + 62 PCs + 3 covariates are more than 64 columns"),
        (["--eigensnp", "--gpca-assoc-pheno", f["dup"]], f"--gpca-assoc-pheno: {f['dup']}:3: sample f0 s0 appears twice"),
        (["--eigensnp", "--gpca-assoc-pheno", f["nohead"]], f"--gpca-assoc-pheno: {f['nohead']}: the header `FID IID name...` with at least one column is required"),
        (["--eigensnp", "--gpca-assoc-pheno", f["word"]], f"--gpca-assoc-pheno: {f['word']}:2: `1_0` is not a number"),
        (["--eigensnp", "--gpca-assoc-pheno", f["absent"]], f"--gpca-assoc-pheno: cannot open {f['absent']}"),
        (E + ["--gpca-assoc-covar", f["dup"]], f"--gpca-assoc-covar: {f['dup']}:3: sample f0 s0 appears twice"),
    ]


def test_flag_errors_python(tmp_path):
    f = pheno_files(tmp_path)
    for flags, msg in bad_flags(f):
        with pytest.raises(SystemExit) as ei:
            main(BASE + flags)
        assert str(ei.value).startswith("error: ") and msg in str(ei.value), (flags, str(ei.value))
    # accepted flags get as far as the missing fileset: 60 traits + 4 PCs = 64 columns, P = 0, P = k-global
    for ok in (["--gpca-assoc-pheno", f["wide"], "--gpca-assoc-pcs", "4"], ["--gpca-assoc-pheno", f["ok"], "--gpca-assoc-pcs", "0", "--gpca-assoc-vif", "1"],
               ["--gpca-assoc-pheno", f["ok"], "--gpca-assoc-pcs", "10", "--gpca-assoc-covar", f["cov"]]):
        with pytest.raises(FileNotFoundError) as ei:
            main(BASE + ["--eigensnp"] + ok)
        assert "t.fam" in str(ei.value) or "t.bed" in str(ei.value), str(ei.value)


def test_cpp_twins_match_python(tmp_path):
    """formats.hpp against io.py: read_pheno (values and refusals), align_pheno, assoc_bands, the writer's bytes"""
    src = tmp_path / "drv.cpp"
    src.write_text(r"""
#include "formats.hpp"
#include <iostream>
int main(int argc, char** argv) {
    for (int i = 2; i < argc; ++i) {
        try {
            const gpca_host::PhenoTable t = gpca_host::read_pheno(argv[i]);
            std::printf("T");
            for (const auto& n : t.names) std::printf(" %s", n.c_str());
            const auto a = gpca_host::align_pheno(t, {"f0", "f1", "f2", "f3", "fx"}, {"s0", "s1", "s2", "s3", "s0"});
            for (double v : a) std::printf(" %.17g", v);
            std::printf("\n");
        } catch (const std::runtime_error& e) { std::printf("E %s\n", e.what()); }
    }
    for (auto kl : {std::pair<int64_t, int64_t>{0, 5}, {10, 64}, {1000, 33}, {200000000, 64}, {5, 0}}) {
        std::printf("B");
        for (auto b : gpca_host::assoc_bands(kl.first, kl.second)) std::printf(" %lld:%lld", (long long)b.first, (long long)b.second);
        std::printf("\n");
    }
    for (auto b : gpca_host::assoc_bands(10, 64, 256)) std::printf("b %lld:%lld\n", (long long)b.first, (long long)b.second);
    const double nan = std::nan("");
    gpca_host::ensure_parent(argv[1]);
    gpca_host::AssocWriter w(argv[1], "height");
    w.add_row("1", 100, "rs1", "A", 500.0, 0.25, 1.5, 0.5, 3.0, 2.56789012);
    w.add_row("1", 2500000, "rs2", "G", 499.0, 0.123456789, -2.5e-7, 1e-7, -2.5, 1234.5678);
    w.add_row("X", 7, "rs3", "T", 0.0, nan, nan, nan, nan, nan);
    w.add_row("2", 9, "rs4", "C", 12.0, 0.5, 1e10, 123456789.0, 0.0, INFINITY);
    return 0;
}
""")
    exe = str(tmp_path / "drv")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "genomic_pca_amd", "host"), str(src), "-lz", "-o", exe])
    files = [_write(tmp_path / "a.pheno", "FID IID height bmi\nf2 s2 1.5 NA\nf0 s0 -2 3e1\n\nf9 s9 7 8\nf1 s1 nan 0.25\n"),
             _write(tmp_path / "h.pheno", "#FID\tIID\ty\nf3 s3 +.5\nf0 s0 inf\nf1 s1 NaN\n"),
             _write(tmp_path / "d.pheno", "FID IID y\nf0 s0 1\nf1 s1 2\nf0 s0 3\n"), _write(tmp_path / "n.pheno", "f0 s0 1\nf1 s1 2\n"),
             _write(tmp_path / "e.pheno", "FID IID\nf0 s0\n"), _write(tmp_path / "s.pheno", "FID IID y\nf0 s0 1 2\n"),
             _write(tmp_path / "x.pheno", "FID IID y\nf0 s0 tall\n"), _write(tmp_path / "r.pheno", "FID IID y y\nf0 s0 1 2\n"),
             _write(tmp_path / "hex.pheno", "FID IID y\nf0 s0 0x10\n"), _write(tmp_path / "empty.pheno", "\n\n")]
    want = []
    for p in files:
        try:
            t = gio.read_pheno(p)
            a = gio.align_pheno(t, ["f0", "f1", "f2", "f3", "fx"], ["s0", "s1", "s2", "s3", "s0"])
            want.append(" ".join(["T", *t.names, *("%.17g" % v for v in a.ravel())]))
        except ValueError as e:
            want.append(f"E {e}")
    for K, L in ((0, 5), (10, 64), (1000, 33), (200000000, 64), (5, 0)):
        want.append(" ".join(["B", *(f"{a}:{b}" for a, b in gio.assoc_bands(K, L))]))
    want += [f"b {a}:{b}" for a, b in gio.assoc_bands(10, 64, 256)]
    pre_c, pre_p = str(tmp_path / "c" / "run"), str(tmp_path / "p" / "run")
    out = subprocess.run([exe, pre_c, *files], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[:-1] == want and sum(w.startswith("E ") for w in want) == 8
    nan = float("nan")
    gio.write_assoc(pre_p, "height", ["1", "1", "X", "2"], [100, 2500000, 7, 9], ["rs1", "rs2", "rs3", "rs4"], ["A", "G", "T", "C"],
                    [500.0, 499.0, 0.0, 12.0], [0.25, 0.123456789, nan, 0.5], [1.5, -2.5e-7, nan, 1e10], [0.5, 1e-7, nan, 123456789.0],
                    [3.0, -2.5, nan, 0.0], [2.56789012, 1234.5678, nan, float("inf")])
    assert open(pre_c + ".height.assoc.linear", "rb").read() == open(pre_p + ".height.assoc.linear", "rb").read()
