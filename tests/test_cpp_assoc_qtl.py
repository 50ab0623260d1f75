"""Both command lines with --gpca-qtl-pheno: --eigensnp on the synthetic .bed of tests/test_cpp_assoc_score.py (two populations with
planted relatives) with 40 traits, 3 PCs and a covariate file, --gpca-king-cutoff, and a threshold low enough for a few hundred hits.
The two programs write byte-identical P.qtl.hits and P.qtl.best; the hits are in (SNP, trait) order and are the pairs whose LOG10P
reaches the threshold in P.<trait>.assoc.linear of the association scan run on the same traits (39 of them: that scan holds 64 columns),
with the same statistics, character for character; the trait planted on a SNP has that SNP as its best; a run without the flags writes
the same set of files with the same bytes as before, and the run with them adds the two files and moves no byte of the others.  The
refusals give the same messages in both programs (no GPU: the arguments are refused before any work on the device)."""
import os
import subprocess

import numpy as np
import pytest

from genomic_pca_amd.cli import main
from test_cpp_assoc_score import BIN, K_GLOBAL, ROOT, CAUSAL, fileset, host_bin  # noqa: F401  (fixtures)

T = 40
LOG10P = 2.0


@pytest.fixture(scope="module")
def traits(fileset):
    pre, ld, d, cov, M, N = fileset
    from test_cpp_pcrelate import cohort
    G = cohort()
    rng = np.random.default_rng(7)
    Y = rng.standard_normal((N, T))
    Y[:, 17] += 0.9 * G[CAUSAL]
    path = os.path.join(d, "qtl.pheno")
    with open(path, "w") as f:                                       # shuffled rows; s3 absent; a sample the .fam does not have
        f.write("FID IID " + " ".join(f"g{t}" for t in range(T)) + "\nfam999 s999 " + " ".join(["0"] * T) + "\n")
        for i in rng.permutation(N):
            if i != 3:
                f.write(f"fam{i // 4} s{i} " + " ".join(repr(float(v)) for v in Y[i]) + "\n")
    return path


def base_args(fileset):
    pre, ld, d, cov, M, N = fileset
    return ["--eigensnp", "--bed-file", pre + ".bed", "--ld-block-file", ld, "--eigensnp-k-global", str(K_GLOBAL), "--eigensnp-max-hwe-p", "1.0",
            "--gpca-king-cutoff", "0.0884"]


@pytest.mark.gpu
def test_both_clis_qtl(tmp_path, host_bin, fileset, traits):
    pre, ld, d, cov, M, N = fileset
    qtl = ["--gpca-qtl-pheno", traits, "--gpca-qtl-pcs", "3", "--gpca-qtl-covar", cov, "--gpca-qtl-log10p", str(LOG10P)]
    out_py, out_c, out_t, out_plain, out_a = (str(tmp_path / n / "P") for n in ("py", "c", "ct", "plain", "assoc"))
    assert main(base_args(fileset) + qtl + ["--out", out_py]) == 0
    r = subprocess.run([host_bin, *base_args(fileset), *qtl, "--out", out_c], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "QTL scan of" in r.stderr
    for ext in (".qtl.hits", ".qtl.best", ".eigensnp.pca.tsv"):
        assert open(out_py + ext, "rb").read() == open(out_c + ext, "rb").read(), ext
    hits = [ln.split("\t") for ln in open(out_c + ".qtl.hits").read().split("\n")[1:-1]]
    best = [ln.split("\t") for ln in open(out_c + ".qtl.best").read().split("\n")[1:-1]]
    assert open(out_c + ".qtl.hits").readline() == "#CHROM\tPOS\tID\tA1\tTRAIT\tOBS_CT\tA1_FREQ\tBETA\tSE\tT_STAT\tLOG10P\n"
    assert 50 < len(hits) < 20000 and len(best) == T and [b[0] for b in best] == [f"g{t}" for t in range(T)]
    key = [(int(h[1]), int(h[4][1:])) for h in hits]
    assert key == sorted(key) and len(set(key)) == len(key)                       # (position = row + 1 in this fileset)
    assert all(float(h[10]) >= LOG10P * (1 - 1e-5) for h in hits)                   # (%.6g of a value at or beyond the threshold)
    b17 = best[17]
    assert b17[3] == f"rs{CAUSAL}" and float(b17[8]) > 6 and len({b[9] for b in best}) == 1 and int(b17[9]) > 1000
    # the same threshold as |t|: the same files
    import genomic_pca_amd as gpca
    import re
    n_inc = int(re.search(r"on (\d+) of \d+ samples", r.stderr).group(1))
    tmin = gpca.qtl_t_min(LOG10P, n_inc - 4 - 2)
    r = subprocess.run([host_bin, *base_args(fileset), *qtl[:6], "--gpca-qtl-t", repr(tmin), "--out", out_t], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for ext in (".qtl.hits", ".qtl.best"):
        assert open(out_t + ext, "rb").read() == open(out_c + ext, "rb").read(), ext
    # the association scan on the first 39 traits with the same covariates: a hit's line is that scan's line of the SNP, and every
    # line of that scan at or beyond the threshold is a hit
    sub = os.path.join(d, "qtl39.pheno")
    with open(traits) as f, open(sub, "w") as g:
        g.writelines(" ".join(ln.split()[:2 + 39]) + "\n" for ln in f)
    r = subprocess.run([host_bin, *base_args(fileset), "--gpca-assoc-pheno", sub, "--gpca-assoc-pcs", "3", "--gpca-assoc-covar", cov, "--out", out_a],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    by_pair = {(h[2], h[4]): h for h in hits}
    n_seen = 0
    for t in range(39):
        for ln in open(out_a + f".g{t}.assoc.linear").read().split("\n")[1:-1]:
            a = ln.split("\t")
            h = by_pair.get((a[2], f"g{t}"))
            if h is not None:
                assert h[:4] + h[5:] == a, (h, a)
                n_seen += 1
            else:
                assert a[9] == "NA" or float(a[9]) < LOG10P * (1 + 1e-5), a
        bt = best[t]
        rows = [ln.split("\t") for ln in open(out_a + f".g{t}.assoc.linear").read().split("\n")[1:-1] if ln.split("\t")[2] == bt[3]]
        assert rows and rows[0][:4] == bt[1:5] and rows[0][6:] == bt[5:9], (bt, rows)
    assert n_seen == sum(1 for h in hits if int(h[4][1:]) < 39)
    # without the flags: the files of before, byte for byte; with them: two more files and no other byte moves
    r = subprocess.run([host_bin, *base_args(fileset), "--out", out_plain], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    plain, withq = sorted(os.listdir(os.path.dirname(out_plain))), sorted(os.listdir(os.path.dirname(out_c)))
    assert withq == sorted(plain + ["P.qtl.hits", "P.qtl.best"]) and not any("qtl" in p for p in plain)
    for name in plain:
        assert open(os.path.join(os.path.dirname(out_plain), name), "rb").read() == open(os.path.join(os.path.dirname(out_c), name), "rb").read(), name


BASE = ["--bed-file", "t.bed", "--ld-block-file", "l.txt", "--out", "x"]


def test_qtl_flag_refusals_are_the_same(tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "genomic_pca_amd", "host"), "-s"])
    ph = tmp_path / "p.txt"
    ph.write_text("FID IID a b\nf s 1 2\n")
    wide = tmp_path / "wide.txt"
    wide.write_text("FID IID " + " ".join(f"c{i}" for i in range(62)) + "\nf s " + " ".join(["1"] * 62) + "\n")
    Q = ["--gpca-qtl-pheno", str(ph)]
    cases = [(["--gpca-qtl-pcs", "2"], "need --gpca-qtl-pheno"), (["--gpca-qtl-log10p", "3"], "need --gpca-qtl-pheno"),
             (Q, "needs the --eigensnp workflow"),
             (["--eigensnp", *Q, "--gpca-stream", "on"], "needs the genotype matrix resident on the device"),
             (["--eigensnp", *Q, "--gpca-eigensnp-local-stage"], "cannot be combined with --gpca-eigensnp-local-stage"),
             (["--eigensnp", *Q, "--gpca-qtl-log10p", "3", "--gpca-qtl-t", "4"], "give one"),
             (["--eigensnp", *Q, "--gpca-qtl-log10p", "-1"], "--gpca-qtl-log10p must be finite and at least 0"),
             (["--eigensnp", *Q, "--gpca-qtl-t", "inf"], "--gpca-qtl-t must be finite and at least 0"),
             (["--eigensnp", *Q, "--gpca-qtl-vif", "0.5"], "--gpca-qtl-vif must be finite and at least 1"),
             (["--eigensnp", *Q, "--gpca-qtl-pcs", "99"], "--gpca-qtl-pcs P must lie in"),
             (["--eigensnp", "--gpca-qtl-pheno", str(tmp_path / "none.txt")], "cannot open"),
             (["--eigensnp", *Q, "--gpca-qtl-covar", str(wide), "--gpca-qtl-pcs", "2"], "2 PCs + 62 covariates are more than 63 covariates")]
    for flags, text in cases:
        with pytest.raises(SystemExit) as ei:
            main(BASE + flags)
        r = subprocess.run([BIN, *BASE, *flags], capture_output=True, text=True, timeout=60)
        last = r.stderr.strip().split("\n")[-1]
        assert r.returncode != 0 and last == str(ei.value) and text in last, (flags, last, str(ei.value))
    # the messages of the association scan's refusals, with the flag's own name
    for flags in (["--eigensnp", "--gpca-stream", "on"], ["--eigensnp", "--gpca-eigensnp-local-stage"]):
        with pytest.raises(SystemExit) as eq:
            main(BASE + flags + Q)
        with pytest.raises(SystemExit) as ea:
            main(BASE + flags + ["--gpca-assoc-pheno", str(ph)])
        assert str(eq.value) == str(ea.value).replace("--gpca-assoc-pheno", "--gpca-qtl-pheno")
    helptext = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    for flag in ("--gpca-qtl-pheno", "--gpca-qtl-pcs", "--gpca-qtl-covar", "--gpca-qtl-log10p", "--gpca-qtl-t", "--gpca-qtl-vif"):
        assert flag in helptext
