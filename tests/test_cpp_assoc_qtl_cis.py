"""Both command lines with --gpca-qtl-cis-pos: --eigensnp on the synthetic .bed of tests/test_cpp_assoc_score.py (one chromosome,
position = row + 1) with three traits: g0 follows the SNP at position 1 207 and has its position there, g1 has no position, g2 sits on a
chromosome the SNPs do not have, so its window holds no SNP.  The two programs write a byte-identical P.qtl.cis; g0's line names the
planted SNP with PVAL_PERM = 1 / (P + 1), g1's is a row of NA, g2's has N_VAR = 0 and NA from ID on; --gpca-qtl-cis-perm 0 leaves the
beta columns NA; --gpca-qtl-cis-only writes no trans file; the run with --gpca-qtl-pheno alone writes what it wrote before, and the cis
flags add P.qtl.cis and move no byte of the other files.  The refusals give the same messages in both programs (no GPU: the arguments
are refused before any work on the device)."""
import os
import subprocess

import numpy as np
import pytest

from genomic_pca_amd.cli import main
from test_cpp_assoc_score import BIN, K_GLOBAL, ROOT, CAUSAL, fileset, host_bin  # noqa: F401  (fixtures)

PERM = 200
HEADER = "#TRAIT\tCHROM\tPOS\tN_VAR\tID\tVAR_POS\tA1\tBETA\tSE\tT_STAT\tLOG10P_NOMINAL\tTRUE_DF\tSHAPE1\tSHAPE2\tPVAL_PERM\tLOG10P_BETA"


@pytest.fixture(scope="module")
def traits(fileset):
    pre, ld, d, cov, M, N = fileset
    from test_cpp_pcrelate import cohort
    G = cohort()
    rng = np.random.default_rng(8)
    Y = rng.standard_normal((N, 3))
    Y[:, 0] += 0.9 * G[CAUSAL]
    pheno, pos = os.path.join(d, "cis.pheno"), os.path.join(d, "cis.pos")
    with open(pheno, "w") as f:
        f.write("FID IID g0 g1 g2\n")
        for i in rng.permutation(N):
            if i != 3:
                f.write(f"fam{i // 4} s{i} " + " ".join(repr(float(v)) for v in Y[i]) + "\n")
    with open(pos, "w") as f:
        f.write(f"TRAIT CHROM POS\ng2 2 500\n\ng0 chr1 {CAUSAL + 1}\nother 1 77\n")
    return pheno, pos


def base_args(fileset):
    pre, ld, d, cov, M, N = fileset
    return ["--eigensnp", "--bed-file", pre + ".bed", "--ld-block-file", ld, "--eigensnp-k-global", str(K_GLOBAL), "--eigensnp-max-hwe-p", "1.0",
            "--gpca-king-cutoff", "0.0884"]


@pytest.mark.gpu
def test_both_clis_qtl_cis(tmp_path, host_bin, fileset, traits):
    pre, ld, d, cov, M, N = fileset
    pheno, pos = traits
    qtl = ["--gpca-qtl-pheno", pheno, "--gpca-qtl-pcs", "3", "--gpca-qtl-covar", cov, "--gpca-qtl-log10p", "2"]
    cis = ["--gpca-qtl-cis-pos", pos, "--gpca-qtl-cis-window", "150", "--gpca-qtl-cis-perm", str(PERM), "--gpca-qtl-cis-seed", "5"]
    out_py, out_c, out_only, out_trans, out_nom = (str(tmp_path / n / "P") for n in ("py", "c", "only", "trans", "nom"))
    assert main(base_args(fileset) + qtl + cis + ["--out", out_py]) == 0
    r = subprocess.run([host_bin, *base_args(fileset), *qtl, *cis, "--out", out_c], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "cis-QTL mapping of 2 of 3 traits" in r.stderr
    for ext in (".qtl.cis", ".qtl.hits", ".qtl.best", ".eigensnp.pca.tsv"):
        assert open(out_py + ext, "rb").read() == open(out_c + ext, "rb").read(), ext
    lines = open(out_c + ".qtl.cis").read().split("\n")
    assert lines[0] == HEADER and lines[-1] == "" and len(lines) == 5
    g0, g1, g2 = (ln.split("\t") for ln in lines[1:4])
    assert g0[:3] == ["g0", "chr1", str(CAUSAL + 1)] and g0[4:6] == [f"rs{CAUSAL}", str(CAUSAL + 1)]
    assert 100 < int(g0[3]) <= 301 and float(g0[10]) > 6 and "NA" not in g0
    assert float(g0[14]) == pytest.approx(1.0 / (PERM + 1), rel=1e-5) and float(g0[15]) > 3
    assert g1 == ["g1"] + ["NA"] * 15
    assert g2 == ["g2", "2", "500", "0"] + ["NA"] * 12
    # g0's statistics are the best line of the trans scan, character for character (the planted SNP is the best of all SNPs too)
    best0 = open(out_c + ".qtl.best").read().split("\n")[1].split("\t")
    assert best0[3] == g0[4] and best0[5:9] == g0[7:11]
    # cis only: no trans file; the cis file does not move
    r = subprocess.run([host_bin, *base_args(fileset), *qtl, *cis, "--gpca-qtl-cis-only", "--out", out_only], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "QTL scan of" not in r.stderr
    only = sorted(os.listdir(os.path.dirname(out_only)))
    assert "P.qtl.cis" in only and "P.qtl.hits" not in only and "P.qtl.best" not in only
    assert open(out_only + ".qtl.cis", "rb").read() == open(out_c + ".qtl.cis", "rb").read()
    assert main(base_args(fileset) + qtl + cis + ["--gpca-qtl-cis-only", "--out", str(tmp_path / "pyonly" / "P")]) == 0
    assert sorted(os.listdir(str(tmp_path / "pyonly"))) == only
    # without the cis flags: the files of before; with them: one more file and no other byte moves
    r = subprocess.run([host_bin, *base_args(fileset), *qtl, "--out", out_trans], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    trans, withc = sorted(os.listdir(os.path.dirname(out_trans))), sorted(os.listdir(os.path.dirname(out_c)))
    assert withc == sorted(trans + ["P.qtl.cis"]) and only == sorted(set(trans) - {"P.qtl.hits", "P.qtl.best"} | {"P.qtl.cis"})
    for name in trans:
        assert open(os.path.join(os.path.dirname(out_trans), name), "rb").read() == open(os.path.join(os.path.dirname(out_c), name), "rb").read(), name
    # nominal only: the beta columns are NA, the others do not move
    r = subprocess.run([host_bin, *base_args(fileset), *qtl, *cis[:4], "--gpca-qtl-cis-perm", "0", "--gpca-qtl-cis-only", "--out", out_nom],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    n0 = open(out_nom + ".qtl.cis").read().split("\n")[1].split("\t")
    assert n0[:11] == g0[:11] and n0[11:] == ["NA"] * 5


BASE = ["--bed-file", "t.bed", "--ld-block-file", "l.txt", "--out", "x"]


def test_qtl_cis_flag_refusals_are_the_same(tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "genomic_pca_amd", "host"), "-s"])
    ph = tmp_path / "p.txt"
    ph.write_text("FID IID a b\nf s 1 2\n")
    good = tmp_path / "pos.txt"
    good.write_text("TRAIT CHROM POS\na 1 5\n")
    files = {"head": "GENE CHR POS\na 1 5\n", "short": "TRAIT CHROM POS\na 1\n", "int": "TRAIT CHROM POS\na 1 5.5\n", "empty": ""}
    for name, text in files.items():
        (tmp_path / name).write_text(text)
    Q, P = ["--gpca-qtl-pheno", str(ph)], ["--gpca-qtl-cis-pos", str(good)]
    cases = [(["--eigensnp", *Q, "--gpca-qtl-cis-window", "5"], "need --gpca-qtl-cis-pos"), (["--eigensnp", *Q, "--gpca-qtl-cis-only"], "need --gpca-qtl-cis-pos"),
             (["--eigensnp", *Q, "--gpca-qtl-cis-perm", "5"], "need --gpca-qtl-cis-pos"), (["--eigensnp", *Q, "--gpca-qtl-cis-seed", "5"], "need --gpca-qtl-cis-pos"),
             (["--eigensnp", *P], "--gpca-qtl-cis-pos needs --gpca-qtl-pheno"),
             ([*Q, *P], "needs the --eigensnp workflow"),
             (["--eigensnp", *Q, *P, "--gpca-stream", "on"], "needs the genotype matrix resident on the device"),
             (["--eigensnp", *Q, *P, "--gpca-eigensnp-local-stage"], "cannot be combined with --gpca-eigensnp-local-stage"),
             (["--eigensnp", *Q, *P, "--gpca-qtl-cis-window", "-1"], "--gpca-qtl-cis-window must be at least 0"),
             (["--eigensnp", *Q, *P, "--gpca-qtl-cis-perm", "65536"], "--gpca-qtl-cis-perm must lie in [0, 65535]"),
             (["--eigensnp", *Q, *P, "--gpca-qtl-cis-perm", "-1"], "--gpca-qtl-cis-perm must lie in [0, 65535]"),
             (["--eigensnp", *Q, *P, "--gpca-qtl-cis-seed", "-3"], "--gpca-qtl-cis-seed must be at least 0"),
             (["--eigensnp", *Q, "--gpca-qtl-cis-pos", str(tmp_path / "none.txt")], "cannot open"),
             (["--eigensnp", *Q, "--gpca-qtl-cis-pos", str(tmp_path / "head")], "the header must be 'TRAIT CHROM POS'"),
             (["--eigensnp", *Q, "--gpca-qtl-cis-pos", str(tmp_path / "empty")], "the header must be 'TRAIT CHROM POS'"),
             (["--eigensnp", *Q, "--gpca-qtl-cis-pos", str(tmp_path / "short")], "line 2 does not hold TRAIT CHROM POS"),
             (["--eigensnp", *Q, "--gpca-qtl-cis-pos", str(tmp_path / "int")], "the position '5.5' is not an integer")]
    for flags, text in cases:
        with pytest.raises(SystemExit) as ei:
            main(BASE + flags)
        r = subprocess.run([BIN, *BASE, *flags], capture_output=True, text=True, timeout=60)
        last = r.stderr.strip().split("\n")[-1]
        assert r.returncode != 0 and last == str(ei.value) and text in last, (flags, last, str(ei.value))
    helptext = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    for flag in ("--gpca-qtl-cis-pos", "--gpca-qtl-cis-window", "--gpca-qtl-cis-perm", "--gpca-qtl-cis-seed", "--gpca-qtl-cis-only"):
        assert flag in helptext
