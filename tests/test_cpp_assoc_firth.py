"""Both command lines with --gpca-assoc-firth, on the fileset of tests/test_cpp_assoc_score.py (one case / control trait, one
quantitative trait, a covariate file, --gpca-king-cutoff).  The two programs write byte-identical P.cad.assoc.logistic with the header
that ends in LOG10P FIRTH, and the file is what GpcaEngine.assoc_logistic_firth gives through io.write_assoc_logistic.  Without the
flag the file has the header and the rows it had before the flag existed: it is the flagged file of --gpca-assoc-firth-z inf (no test
corrected: the score test's values everywhere) with the FIRTH column cut off, byte for byte, and the flagged run at the default cutoff
differs from it only in BETA, SE and LOG10P of the rows marked Y; Z_STAT and the linear file of the quantitative trait do not move.
CPU-only: the writer and its twin in host/formats.hpp against a literal file, and the refusals (the flag without
--gpca-assoc-logistic, beside --gpca-assoc-spa, the cutoff without the flag, a negative or NaN cutoff), alike in both programs."""
import math
import os
import subprocess

import numpy as np
import pytest

from genomic_pca_amd import io as gio
from genomic_pca_amd.cli import main
from genomic_pca_amd.engine import GpcaEngine
from test_cpp_assoc_score import BIN, K_GLOBAL, PCS, ROOT, fileset, host_bin  # noqa: F401  (fixtures)

HEAD = "#CHROM\tPOS\tID\tA1\tOBS_CT\tA1_FREQ\tBETA\tSE\tZ_STAT\tLOG10P"
INF = float("inf")


@pytest.mark.gpu
def test_both_clis_assoc_firth(tmp_path, host_bin, fileset, monkeypatch):
    pre, ld, d, cov, M, N = fileset
    args = ["--eigensnp", "--bed-file", pre + ".bed", "--ld-block-file", ld, "--eigensnp-k-global", str(K_GLOBAL), "--eigensnp-max-hwe-p", "1.0",
            "--gpca-assoc-covar", cov, "--gpca-assoc-pcs", str(PCS), "--gpca-king-cutoff", "0.0884", "--gpca-assoc-pheno",
            os.path.join(d, "t12.pheno"), "--gpca-assoc-logistic"]
    seen = []
    real = GpcaEngine.assoc_logistic_firth

    def spy(self, *a, **kw):
        r = real(self, *a, **kw)
        seen.append((kw.get("firth_z"), r))
        return r
    monkeypatch.setattr(GpcaEngine, "assoc_logistic_firth", spy)
    out_py, out_c, out_inf, out_plain = (str(tmp_path / n / "P") for n in ("py", "c", "inf", "plain"))
    assert main(args + ["--gpca-assoc-firth", "--out", out_py]) == 0
    monkeypatch.undo()
    for extra, out in ((["--gpca-assoc-firth"], out_c), (["--gpca-assoc-firth", "--gpca-assoc-firth-z", "inf"], out_inf), ([], out_plain)):
        r = subprocess.run([host_bin, *args, *extra, "--out", out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
    for ext in (".cad.assoc.logistic", ".height.assoc.linear"):
        assert open(out_py + ext, "rb").read() == open(out_c + ext, "rb").read(), ext
    assert open(out_plain + ".height.assoc.linear", "rb").read() == open(out_c + ".height.assoc.linear", "rb").read()
    fir = open(out_c + ".cad.assoc.logistic").read().split("\n")
    inf = open(out_inf + ".cad.assoc.logistic").read().split("\n")
    plain = open(out_plain + ".cad.assoc.logistic").read().split("\n")
    assert fir[0] == inf[0] == HEAD + "\tFIRTH" and plain[0] == HEAD and fir[-1] == inf[-1] == plain[-1] == "" and len(fir) == len(inf) == len(plain) > 100
    # no flag = the cutoff inf without its last column, byte for byte
    assert [ln.rsplit("\t", 1)[0] for ln in inf[:-1]] == plain[:-1]
    assert {ln.rsplit("\t", 1)[1] for ln in inf[1:-1]} <= {"N", "NA"}
    # the default cutoff: only the corrected rows' BETA, SE and LOG10P move; Z_STAT never does
    marks = [ln.rsplit("\t", 1)[1] for ln in fir[1:-1]]
    assert set(marks) <= {"N", "Y", "F", "NA"} and marks.count("Y") > 0 and marks.count("N") > marks.count("Y")
    for a, b, m in zip(fir[1:-1], plain[1:-1], marks):
        fa, fb = a.split("\t"), b.split("\t")
        assert fa[:6] == fb[:6] and fa[8] == fb[8]
        if m == "Y":
            assert abs(float(fa[8])) >= 1.959964 and float(fa[9]) > 0 and float(fa[7]) > 0 and math.isfinite(float(fa[6]))
        else:
            assert fa[6:10] == fb[6:10] and (m == "NA") == (fb[9] == "NA")
    # the file against what the run's own call returned
    assert len(seen) == 1 and seen[0][0] == 1.959964
    res = seen[0][1]
    st = res["firth_status"][:, 0]
    assert marks == ["NA" if v != v else "NYF"[int(s)] for v, s in zip(res["log10p"][:, 0], st)]
    col = lambda j: np.array([float(ln.split("\t")[j]) if ln.split("\t")[j] != "NA" else np.nan for ln in fir[1:-1]])
    assert np.allclose(col(9), res["log10p"][:, 0], rtol=1e-5, equal_nan=True)
    assert np.allclose(col(6), np.where(st == 1, res["firth_beta"][:, 0], res["beta"][:, 0]), rtol=1e-5, equal_nan=True)
    assert np.allclose(col(7), np.where(st == 1, res["firth_se"][:, 0], res["se"][:, 0]), rtol=1e-5, equal_nan=True)


def test_write_assoc_logistic_with_firth_against_a_literal_file(tmp_path):
    prefix = str(tmp_path / "out" / "run")
    nan = float("nan")
    args = (["1", "1", "X", "2"], [100, 2500000, 7, 9], ["rs1", "rs2", "rs3", "rs4"], ["A", "G", "T", "C"], [500.0, 499.0, 0.0, 12.0],
            [0.25, 0.123456789, nan, 0.5], [1.5, -2.5e-7, nan, 1e10], [0.5, 1e-7, nan, 123456789.0], [3.0, -2.5, nan, 0.0],
            [2.56789012, 1234.5678, nan, 0.0])
    path = gio.write_assoc_logistic(prefix, "cad", *args, firth=[1, 2, 0, 0])
    want = ("#CHROM\tPOS\tID\tA1\tOBS_CT\tA1_FREQ\tBETA\tSE\tZ_STAT\tLOG10P\tFIRTH\n"
            "1\t100\trs1\tA\t500\t0.25\t1.5\t0.5\t3\t2.56789\tY\n"
            "1\t2500000\trs2\tG\t499\t0.123457\t-2.5e-07\t1e-07\t-2.5\t1234.57\tF\n"
            "X\t7\trs3\tT\t0\tNA\tNA\tNA\tNA\tNA\tNA\n"
            "2\t9\trs4\tC\t12\t0.5\t1e+10\t1.23457e+08\t0\t0\tN\n")
    assert open(path).read() == want
    plain = gio.write_assoc_logistic(str(tmp_path / "plain" / "run"), "cad", *args)
    assert open(plain).read() == "\n".join(ln.rsplit("\t", 1)[0] for ln in want.split("\n")[:-1]) + "\n"
    with pytest.raises(ValueError):
        gio.write_assoc_logistic(prefix, "cad", *args, firth=[1, 2])
    with pytest.raises(ValueError):
        gio.write_assoc_logistic(prefix, "cad", *args, firth=[1, 2, 0, 0], spa=[1, 2, 0, 0])
    exe = str(tmp_path / "dump_assoc_firth")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "genomic_pca_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp", "dump_assoc_firth.cpp"), "-lz", "-o", exe])
    pre_c = str(tmp_path / "c" / "run")
    out = subprocess.run([exe, pre_c], capture_output=True, text=True, check=True).stdout.split()
    assert open(pre_c + ".cad.assoc.logistic", "rb").read() == want.encode()
    assert out[:-1] == ["%d" % gio.firth_z_ok(v) for v in (0.0, 1.959964, INF, -1e-300, -1.0, math.nan, -INF)] == list("1110000")
    assert out[-1] == "1"                                # the twin refuses both columns at once, too


BASE = ["--bed-file", "t.bed", "--ld-block-file", "l.txt", "--out", "x"]


def test_firth_flag_refusals_are_the_same(tmp_path, host_bin):
    ph = str(tmp_path / "cc.pheno")
    with open(ph, "w") as f:
        f.write("FID IID cc\n" + "".join(f"f{i} s{i} {1 + i % 2}\n" for i in range(6)))
    E = ["--eigensnp", "--gpca-assoc-pheno", ph]
    LF = E + ["--gpca-assoc-logistic", "--gpca-assoc-firth"]
    for flags, msg in ((E + ["--gpca-assoc-firth"], "--gpca-assoc-firth needs --gpca-assoc-logistic"),
                       (LF + ["--gpca-assoc-spa"], "--gpca-assoc-firth and --gpca-assoc-spa exclude each other"),
                       (E + ["--gpca-assoc-firth-z", "3"], "--gpca-assoc-firth-z needs --gpca-assoc-firth"),
                       (E + ["--gpca-assoc-logistic", "--gpca-assoc-firth-z", "3"], "--gpca-assoc-firth-z needs --gpca-assoc-firth"),
                       (LF + ["--gpca-assoc-firth-z", "-0.5"], "--gpca-assoc-firth-z must be at least 0, or inf for no correction"),
                       (LF + ["--gpca-assoc-firth-z", "nan"], "--gpca-assoc-firth-z must be at least 0, or inf for no correction")):
        with pytest.raises(SystemExit) as ei:
            main(BASE + flags)
        assert str(ei.value) == "error: " + msg, (flags, str(ei.value))
        r = subprocess.run([host_bin, *BASE, *flags], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stderr == "error: " + msg + "\n", (flags, r.stderr)
    # accepted values get as far as the missing fileset
    for ok in ([], ["--gpca-assoc-firth-z", "0"], ["--gpca-assoc-firth-z", "inf"], ["--gpca-assoc-firth-z", "2.5"]):
        with pytest.raises(FileNotFoundError):
            main(BASE + LF + ok)
    helptext = subprocess.run([host_bin, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--gpca-assoc-firth" in helptext and "--gpca-assoc-firth-z" in helptext and "no Firth correction" not in helptext
