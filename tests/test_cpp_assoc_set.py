"""Both command lines with --gpca-assoc-set-list, on the fileset of tests/test_cpp_assoc_score.py (one case / control trait, one
quantitative trait, a covariate file, --gpca-king-cutoff).  The set list holds ordinary sets, a set whose every ID the SNP QC removed
(an NA row), a set of 200 variants (an NA row and a note on stderr), a set with an ID that the QC removed and one that no SNP has, and a
set whose variants the MAF rule thins.  The two programs write byte-identical P.cad.assoc.set, one row per set in file order, and the
same note; every other file of the run is byte-identical to a run without the flag; the rows are what GpcaEngine.assoc_logistic_set and
gpca.set_test give for the sets, on the QC mask.
CPU-only: the twins of host/formats.hpp (the set-list reader, the weights, the MAF rule, the grouping, the writer against a literal
file) and the refusals, alike in both programs."""
import math
import os
import subprocess

import numpy as np
import pytest

from genomic_pca_amd import io as gio
from genomic_pca_amd.cli import main
from test_cpp_assoc_score import BIN, K_GLOBAL, PCS, ROOT, fileset, host_bin  # noqa: F401  (fixtures)

HEAD = "#SET\tCHROM\tPOS\tN_VAR\tN_USED\tBURDEN_BETA\tBURDEN_SE\tBURDEN_Z\tBURDEN_LOG10P\tSKAT_Q\tSKAT_LOG10P\tSKAT"


def write_sets(path, kept):
    """kept: the IDs of the QC-kept SNPs in order (rs300 .. rs319 are not among them)"""
    ids = lambda rows: ",".join(f"rs{i}" for i in rows)
    assert not {f"rs{i}" for i in range(300, 320)} & set(kept)
    with open(path, "w") as f:
        f.write("# name chrom pos variants\n")
        f.write(f"GENE_A 1 11 {','.join(kept[10:30])}\n")
        f.write(f"EMPTY 1 301 {ids(range(300, 320))}\n")                       # dropped by the call-rate filter
        f.write("\n")
        f.write(f"BIG\t1\t401\t{','.join(kept[400:550])}\n")
        f.write(f"MIXED 1 296 {kept[296]},{kept[297]},rs305,{kept[298]},{kept[296]},rs_nobody\n")
        f.write(f"CAUSAL 1 1200 {ids(range(1196, 1216))}\n")
        f.write(f"FULL 1 700 {','.join(kept[700:764])},rs310,{','.join(kept[764:828])}\n")


@pytest.mark.gpu
def test_both_clis_assoc_set(tmp_path, host_bin, fileset, capsys):
    from genomic_pca_amd import _lib
    from genomic_pca_amd.engine import GpcaEngine
    import genomic_pca_amd as gpca
    from test_cpp_assoc_score import gio_qc
    pre, ld, d, cov, M, N = fileset
    fs = gio.read_plink(pre + ".bed")
    with GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=_lib.STORE_INT8) as eng:
        eng.upload_bed2bit(fs.bed_rows, fs.n_samples)
        st = eng.snp_stats(gio_qc())
    kept = np.flatnonzero(st["keep"])
    kept_ids = [fs.variant_ids[i] for i in kept]
    n_causal = len({f"rs{i}" for i in range(1196, 1216)} & set(kept_ids))
    assert 2 <= n_causal <= 20 and len(kept_ids) > 900
    sets = str(tmp_path / "genes.txt")
    write_sets(sets, kept_ids)
    args = ["--eigensnp", "--bed-file", pre + ".bed", "--ld-block-file", ld, "--eigensnp-k-global", str(K_GLOBAL), "--eigensnp-max-hwe-p", "1.0",
            "--gpca-assoc-covar", cov, "--gpca-assoc-pcs", str(PCS), "--gpca-king-cutoff", "0.0884", "--gpca-assoc-pheno",
            os.path.join(d, "t12.pheno"), "--gpca-assoc-logistic", "--gpca-assoc-spa"]
    flag = ["--gpca-assoc-set-list", sets, "--gpca-assoc-set-max-maf", "0.5"]
    out_py, out_c, out_plain, out_maf = (str(tmp_path / n / "P") for n in ("py", "c", "plain", "maf"))
    capsys.readouterr()
    assert main(args + flag + ["--out", out_py]) == 0
    err_py = capsys.readouterr().err
    runs = {}
    for extra, out in ((flag, out_c), ([], out_plain), (flag[:2] + ["--gpca-assoc-set-max-maf", "0.2", "--gpca-assoc-set-weights", "flat"], out_maf)):
        r = subprocess.run([host_bin, *args, *extra, "--out", out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        runs[out] = r.stderr
    note = "note: --gpca-assoc-set-list: set BIG keeps 150 variants, more than 128: NA\n"
    assert note in err_py and note in runs[out_c] and "set tests of 4 of 6 sets" in err_py and "set tests of 4 of 6 sets" in runs[out_c]
    assert open(out_py + ".cad.assoc.set", "rb").read() == open(out_c + ".cad.assoc.set", "rb").read()
    # every other file: what the run without the flag writes, in both programs
    files = lambda out: sorted(f for f in os.listdir(os.path.dirname(out)) if not f.endswith(".assoc.set"))
    assert files(out_py) == files(out_c) == files(out_plain) and len(files(out_c)) >= 4
    assert sorted(os.listdir(os.path.dirname(out_c))) == sorted(files(out_c) + ["P.cad.assoc.set"])
    for f in files(out_plain):
        want = open(os.path.join(os.path.dirname(out_plain), f), "rb").read()
        for out in (out_py, out_c):
            assert open(os.path.join(os.path.dirname(out), f), "rb").read() == want, (f, out)
    # the table
    lines = open(out_c + ".cad.assoc.set").read().split("\n")
    assert lines[0] == HEAD and lines[-1] == "" and len(lines) == 8
    rows = [ln.split("\t") for ln in lines[1:-1]]
    assert [r[0] for r in rows] == ["GENE_A", "EMPTY", "BIG", "MIXED", "CAUSAL", "FULL"] and [r[2] for r in rows] == ["11", "301", "401", "296", "1200", "700"]
    assert rows[1][3:] == ["0"] + ["NA"] * 8 and rows[2][3:] == ["150"] + ["NA"] * 8
    assert rows[0][3] == "20" and rows[3][3] == "3" and rows[4][3] == str(n_causal) and rows[5][3] == "128"
    for r in (rows[0], rows[3], rows[4], rows[5]):
        assert 1 <= int(r[4]) <= int(r[3]) and r[11] in ("Y", "N", "F") and all(math.isfinite(float(v)) for v in r[5:11])
        assert float(r[6]) > 0 and float(r[8]) >= 0 and float(r[9]) >= 0 and float(r[10]) >= 0
    # the MAF rule and the weights change the table, not its shape
    thin = [ln.split("\t") for ln in open(out_maf + ".cad.assoc.set").read().split("\n")[1:-1]]
    assert [r[0] for r in thin] == [r[0] for r in rows] and all(int(a[3]) <= int(b[3]) for a, b in zip(thin, rows))
    assert sum(int(r[3]) for r in thin) < sum(int(r[3]) for r in rows) and thin[2][3] != "150"

    # the rows against calls of the test's own on the QC mask
    seen = []
    real = GpcaEngine.assoc_logistic_set

    def spy(self, Y, sets, covar=None, include=None, max_vif=50.0, ua=False):
        seen.append((np.array(Y), np.array(covar), np.array(include, bool), [np.array(s) for s in sets]))
        return real(self, Y, sets, covar, include, max_vif, ua)
    mp = pytest.MonkeyPatch()
    mp.setattr(GpcaEngine, "assoc_logistic_set", spy)
    try:
        assert main(args + flag + ["--out", str(tmp_path / "again" / "P")]) == 0
    finally:
        mp.undo()
    assert len(seen) == 1 and [len(s) for s in seen[0][3]] == [20, 3, n_causal, 128]
    Y, C, inc, ss = seen[0]
    with GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=_lib.STORE_INT8) as eng:
        eng.upload_bed2bit(fs.bed_rows, fs.n_samples)
        eng.snp_stats(gio_qc())
        eng.set_standardization(st["mu"], st["sigma"], st["keep"])
        assert ss[1].tolist() == [296, 297, 298] and ss[3].tolist() == list(range(700, 828))
        r = eng.assoc_logistic_set(Y, ss, C, include=inc, ua=True)
    for k, row in zip(range(4), (rows[0], rows[3], rows[4], rows[5])):
        lo, hi = r["set_off"][k], r["set_off"][k + 1]
        t = gpca.set_test(np.where(r["flipped"][lo:hi] == 1, -1.0, 1.0) * r["ua"][lo:hi, 0, 0], r["phi"][k][0], gio.set_weights(r["a1_freq"][lo:hi], "beta"))
        got = [float(v) for v in row[5:11]]
        want = [t[n] for n in ("burden_beta", "burden_se", "burden_z", "burden_log10p", "skat_q", "skat_log10p")]
        assert int(row[4]) == t["m_used"] and row[11] == "NYF"[t["skat_status"]] and np.allclose(got, want, rtol=1e-5, atol=0), (row, t)


def test_twins_of_the_set_helpers(tmp_path):
    sets = str(tmp_path / "genes.txt")
    kept = [f"rs{i}" for i in list(range(0, 300)) + list(range(320, 1200))]
    write_sets(sets, kept)
    kept = kept + [kept[296]]                                                           # (a repeated ID means its first row)
    got = gio.read_set_list(sets, kept)
    assert [s.name for s in got] == ["GENE_A", "EMPTY", "BIG", "MIXED", "CAUSAL", "FULL"] and got[2].chrom == "1" and got[2].pos == 401
    assert got[0].rows.tolist() == list(range(10, 30)) and got[1].rows.size == 0 and got[3].rows.tolist() == [296, 297, 298]
    assert got[2].rows.tolist() == list(range(400, 550)) and got[4].rows.tolist() == list(range(1176, 1180)) and got[5].rows.tolist() == list(range(700, 828))
    exe = str(tmp_path / "dump_assoc_set")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "genomic_pca_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp", "dump_assoc_set.cpp"), "-lz", "-o", exe])
    pre_c = str(tmp_path / "c" / "run")
    out = subprocess.run([exe, pre_c, sets, *kept], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[:6] == [" ".join(["set", s.name, s.chrom, str(s.pos)] + [str(r) for r in s.rows]) for s in got]
    freqs = [0.0, 0.001, 0.01, 0.25, 0.5, 0.75, 0.999, 1.0]
    wb, wf = gio.set_weights(freqs, "beta"), gio.set_weights(freqs, "flat")
    ok1, ok5 = gio.set_maf_ok(freqs, 0.01), gio.set_maf_ok(freqs, 0.5)
    assert out[6:14] == ["w %.17g %.17g %d %d" % (wb[i], wf[i], ok1[i], ok5[i]) for i in range(8)]
    assert wb[0] == 25.0 and abs(wb[2] - 25 * 0.99 ** 24) < 1e-13 and wb[3] == wb[5] and ok1.tolist() == [True, True, True, False, False, False, True, True]
    assert out[14] == "w nan %d" % gio.set_maf_ok([math.nan], 0.5)[0] == "w nan 0"
    sizes = [128, 1, 64, 128, 128, 3, 100, 7]
    k = 15
    for mv in (1 << 26, 20000, 9000, 1):
        for T in (1, 3):
            groups = gio.assoc_set_groups(sizes, T, 2, mv)
            assert out[k] == f"groups {mv} {T}:" + "".join(f" {a}-{b}" for a, b in groups), (out[k], groups)
            assert groups[0][0] == 0 and groups[-1][1] == len(sizes) and all(a[1] == b[0] for a, b in zip(groups, groups[1:]))
            for a, b in groups:                       # a group fits, or is a single set
                m = sizes[a:b]
                assert b - a == 1 or (sum(m) * T * 5 <= mv and sum(x * (x + 1) // 2 for x in m) * T <= mv)
            k += 1
    assert gio.assoc_set_groups(sizes, 1, 2) == [(0, 8)] and gio.assoc_set_groups([], 1, 2) == []
    # the writer against a literal file
    nan = math.nan
    keys = ("m_used", "burden_beta", "burden_se", "burden_z", "burden_log10p", "skat_q", "skat_log10p", "skat_status", "z_q", "zeta")
    res = [dict(zip(keys, v)) for v in ([20, 0.0123456789, 0.5, 2.5, 1.90625, 123456.789, 31.25, 1, 8.0, 0.01],
                                        [3, -2.5e-7, 1e-7, -2.5, 1234.5678, 1e-10, 0.0, 0, -0.5, nan],
                                        [0, nan, nan, nan, nan, nan, nan, 0, nan, nan], [2, 1.0, 1.0, 1.0, 0.5, 4.0, 2.0, 2, 1.0, 0.1])]
    path = gio.write_assoc_set(str(tmp_path / "py" / "run"), "cad", ["GENE1", "GENE2", "EMPTY", "ODD", "ODD", "ODD"], ["1", "X", "2", "3", "3", "3"],
                               [1000, 2500000, 7, 9, 9, 9], [20, 5, 0, 2, 200, 2], [res[0], res[1], None, res[2], None, res[3]])
    want = (HEAD + "\n"
            "GENE1\t1\t1000\t20\t20\t0.0123457\t0.5\t2.5\t1.90625\t123457\t31.25\tY\n"
            "GENE2\tX\t2500000\t5\t3\t-2.5e-07\t1e-07\t-2.5\t1234.57\t1e-10\t0\tN\n"
            "EMPTY\t2\t7\t0\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n"
            "ODD\t3\t9\t2\t0\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n"
            "ODD\t3\t9\t200\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n"
            "ODD\t3\t9\t2\t2\t1\t1\t1\t0.5\t4\t2\tF\n")
    assert open(path).read() == want and open(pre_c + ".cad.assoc.set", "rb").read() == want.encode()
    with pytest.raises(ValueError):
        gio.write_assoc_set(str(tmp_path / "py" / "run"), "cad", ["A"], ["1"], [1], [1], [])
    # malformed lists: the same text from both readers
    for text, msg in (("G1 1 100\n", "`NAME CHROM POS ID1,ID2,...` is required"), ("G1 1 100 rs1\nG2 1 x12 rs2\n", "`x12` is not a position"),
                      ("G1 1 1_0 rs1\n", "`1_0` is not a position"), ("G1 1 1234567890123456789 rs1\n", "`1234567890123456789` is not a position"),
                      ("G1 1 \u0661\u0662 rs1\n", "`\u0661\u0662` is not a position"), ("G1 1 - rs1\n", "`-` is not a position"), ("G1 1 100 rs1 extra\n", "`NAME CHROM POS ID1,ID2,...` is required")):
        bad = str(tmp_path / "bad.txt")
        with open(bad, "w", encoding="utf-8") as f:
            f.write(text)
        with pytest.raises(ValueError) as ei:
            gio.read_set_list(bad, kept)
        ln = 2 if "x12" in text else 1
        assert str(ei.value) == f"{bad}:{ln}: {msg}"
        o = subprocess.run([exe, pre_c, bad, *kept[:3]], capture_output=True, text=True, encoding="utf-8", check=True).stdout.split("\n")
        assert f"error {bad}:{ln}: {msg}" in o, o


BASE = ["--bed-file", "t.bed", "--ld-block-file", "l.txt", "--out", "x"]


def test_set_flag_refusals_are_the_same(tmp_path, host_bin):
    ph = str(tmp_path / "cc.pheno")
    with open(ph, "w") as f:
        f.write("FID IID cc\n" + "".join(f"f{i} s{i} {1 + i % 2}\n" for i in range(6)))
    good, bad, missing = str(tmp_path / "genes.txt"), str(tmp_path / "bad.txt"), str(tmp_path / "nowhere.txt")
    write_sets(good, [f"rs{i}" for i in range(320, 1200)])
    with open(bad, "w") as f:
        f.write("G1 1 100 rs1\nG2 1 100\n")
    E = ["--eigensnp", "--gpca-assoc-pheno", ph]
    LS = E + ["--gpca-assoc-logistic", "--gpca-assoc-set-list", good]
    for flags, msg in ((E + ["--gpca-assoc-set-list", good], "--gpca-assoc-set-list needs --gpca-assoc-logistic"),
                       (["--eigensnp", "--gpca-assoc-set-list", good], "--gpca-assoc-set-list needs --gpca-assoc-logistic"),
                       (["--eigensnp", "--gpca-assoc-logistic", "--gpca-assoc-set-list", good], "--gpca-assoc-logistic needs --gpca-assoc-pheno"),
                       (E + ["--gpca-assoc-logistic", "--gpca-assoc-set-max-maf", "0.1"], "--gpca-assoc-set-max-maf and --gpca-assoc-set-weights need --gpca-assoc-set-list"),
                       (E + ["--gpca-assoc-set-weights", "flat"], "--gpca-assoc-set-max-maf and --gpca-assoc-set-weights need --gpca-assoc-set-list"),
                       (LS + ["--gpca-assoc-set-max-maf", "0"], "--gpca-assoc-set-max-maf must lie in (0, 0.5]"),
                       (LS + ["--gpca-assoc-set-max-maf", "0.51"], "--gpca-assoc-set-max-maf must lie in (0, 0.5]"),
                       (LS + ["--gpca-assoc-set-max-maf", "nan"], "--gpca-assoc-set-max-maf must lie in (0, 0.5]"),
                       (LS + ["--gpca-assoc-set-weights", "madsen"], "--gpca-assoc-set-weights must be beta or flat"),
                       (LS[:-1] + [bad], f"--gpca-assoc-set-list: {bad}:2: `NAME CHROM POS ID1,ID2,...` is required"),
                       (LS[:-1] + [missing], f"--gpca-assoc-set-list: cannot open {missing}"),
                       (["--gpca-assoc-pheno", ph, "--gpca-assoc-logistic", "--gpca-assoc-set-list", good], "--gpca-assoc-pheno needs the --eigensnp workflow"),
                       (LS + ["--gpca-stream", "on"], None)):
        with pytest.raises(SystemExit) as ei:
            main(BASE + flags)
        r = subprocess.run([host_bin, *BASE, *flags], capture_output=True, text=True, timeout=60)
        if msg is None:                               # (wherever --gpca-assoc-logistic is refused: the same text, whatever it says)
            assert r.returncode == 2 and r.stderr == str(ei.value) + "\n" and "resident" in r.stderr
            continue
        assert str(ei.value) == "error: " + msg, (flags, str(ei.value))
        assert r.returncode == 2 and r.stderr == "error: " + msg + "\n", (flags, r.stderr)
    # accepted values get as far as the missing fileset
    for ok in ([], ["--gpca-assoc-set-max-maf", "0.5"], ["--gpca-assoc-set-weights", "beta"], ["--gpca-assoc-spa"], ["--gpca-assoc-firth"]):
        with pytest.raises(FileNotFoundError):
            main(BASE + LS + ok)
    helptext = subprocess.run([host_bin, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert all(w in helptext for w in ("--gpca-assoc-set-list", "--gpca-assoc-set-max-maf", "--gpca-assoc-set-weights"))
