"""The two command lines on the LD-score path: the flag rules of --gpca-ld-score and --gpca-assoc-ldsc from both programs without a GPU;
on the GPU, a small synthetic .bed with two chromosomes, missing calls, a quantitative and a case / control trait: byte-identical
P.l2.ldscore, P.l2.M, P.l2.M_5_50 and P.ldsc.summary from the two programs, the L2 column equal to 1 + score 2^-40 from the Python API
printed with %.6g, and every other output file byte-identical to a run without the new flags."""
import os
import subprocess

import numpy as np
import pytest

import genomic_pca_amd as gpca_pkg
from genomic_pca_amd import io as gio
from genomic_pca_amd.cli import main

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "genomic_pca_amd", "bin", "genomic_pca")
BASE = ["--bed-file", "t.bed", "--ld-block-file", "l.txt", "--out", "x"]
RESIDENT = "--gpca-ld-score needs the genotype matrix resident on the device"
BAD_FLAGS = [
    (["--gpca-ld-score", "1000kb"], "--gpca-ld-score needs the --eigensnp workflow"),
    (["--eigensnp", "--gpca-ld-score", "wide"], "--gpca-ld-score: bad LD window 'wide'"),
    (["--eigensnp", "--gpca-ld-score", "1"], "--gpca-ld-score: bad LD window '1'"),
    (["--eigensnp", "--gpca-ld-score", "0kb"], "--gpca-ld-score: bad LD window '0kb'"),
    (["--eigensnp", "--gpca-ld-score", "100kb", "--gpca-stream", "on"], RESIDENT),
    (["--eigensnp", "--gpca-assoc-ldsc"], "--gpca-assoc-ldsc needs --gpca-ld-score and --gpca-assoc-pheno"),
    (["--eigensnp", "--gpca-assoc-ldsc", "--gpca-ld-score", "100kb"], "--gpca-assoc-ldsc needs --gpca-ld-score and --gpca-assoc-pheno"),
]


@pytest.fixture(scope="module")
def host_bin(gpca):
    gpca.load()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "genomic_pca_amd", "host"), "-s"])
    return BIN


@pytest.mark.parametrize("flags,msg", BAD_FLAGS)
def test_flag_errors_are_the_same_from_both_programs(host_bin, flags, msg):
    with pytest.raises(SystemExit) as ei:
        main(BASE + flags)
    text = str(ei.value)
    assert text.startswith("error: ") and msg in text
    r = subprocess.run([host_bin, *BASE, *flags], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and r.stderr.strip() == text, (r.stderr, text)


def test_help_names_the_flags(host_bin):
    out = subprocess.run([host_bin, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--gpca-ld-score <WINDOW>" in out and "--gpca-assoc-ldsc" in out


@pytest.mark.gpu
def test_both_programs_write_the_same_ld_score_files(tmp_path, host_bin):
    rng = np.random.default_rng(91)
    M, N = 1500, 300
    n1 = 800
    p = rng.uniform(0.03, 0.5, size=(M, 1))
    G = (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)
    for i in range(1, M):
        if i % 12 and i != n1:
            cp = rng.random(N) < 0.8
            G[i, cp] = G[i - 1, cp]
    chrom = ["1"] * n1 + ["2"] * (M - n1)
    pos = list(range(1000, 1000 + n1 * 100, 100)) + list(range(500, 500 + (M - n1) * 100, 100))
    # the LD blocks end at 60 000 bp on both chromosomes; the SNPs beyond them pass the SNP QC, stay out of the PCA (which refuses a kept
    # SNP with a missing call) and enter the LD scores and the scans: the missing calls go there
    outside = np.array([q > 60000 for q in pos])
    miss = (rng.random((M, N)) < 0.01) & outside[:, None]
    G[miss] = -127
    ids = [f"s{i}" for i in range(N)]
    pre = str(tmp_path / "in")
    gio.write_plink(pre, G, ids, [f"rs{i}" for i in range(M)], chrom, pos)
    ld = tmp_path / "ld.txt"
    ld.write_text("1 1 30000\n1 30001 60000\n2 1 60000\n")
    causal = rng.choice(M, 150, replace=False)
    g = np.where(G[causal] < 0, 0, G[causal]).astype(np.float64)
    score = (g - g.mean(1, keepdims=True)).T @ rng.standard_normal(150) * 0.15
    quant = score + rng.standard_normal(N)
    case = (score + rng.standard_normal(N) > 0.2).astype(int)
    with open(tmp_path / "ph.txt", "w") as f:
        f.write("FID IID height case\n")
        for i, s in enumerate(ids):
            f.write(f"{s} {s} {'NA' if i % 50 == 7 else repr(float(quant[i]))} {1 + case[i]}\n")
    common = ["--eigensnp", "--bed-file", pre + ".bed", "--ld-block-file", str(ld), "--eigensnp-k-global", "3", "--eigensnp-max-hwe-p", "1.0",
              "--gpca-assoc-pheno", str(tmp_path / "ph.txt"), "--gpca-assoc-logistic"]
    new = ["--gpca-ld-score", "20kb", "--gpca-assoc-ldsc"]
    outs = {}
    for name, args in (("py", common + new), ("py0", common)):
        outs[name] = str(tmp_path / name / "P")
        assert main(args + ["--out", outs[name]]) == 0
    for name, args in (("c", common + new), ("c0", common)):
        outs[name] = str(tmp_path / name / "P")
        r = subprocess.run([host_bin, *args, "--out", outs[name]], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        if name == "c":
            assert "LD scores (window 20kb)" in r.stderr and "LD-score regression of 2 traits" in r.stderr
    new_ext = [".l2.ldscore", ".l2.M", ".l2.M_5_50", ".ldsc.summary"]
    for ext in new_ext:                                                      # the two programs agree byte for byte
        assert open(outs["py"] + ext, "rb").read() == open(outs["c"] + ext, "rb").read(), ext
    # every other output file is what it is without the new flags
    for with_new, without in (("py", "py0"), ("c", "c0")):
        d1, d0 = os.path.dirname(outs[with_new]), os.path.dirname(outs[without])
        f1 = sorted(f for f in os.listdir(d1) if not any(f.endswith(e) for e in new_ext))
        assert f1 == sorted(os.listdir(d0)) and len(f1) >= 5, (f1, sorted(os.listdir(d0)))
        for f in f1:
            assert open(os.path.join(d1, f), "rb").read() == open(os.path.join(d0, f), "rb").read(), f
    # the L2 column against the Python API on the same rows
    fs = gio.read_plink(pre + ".bed")
    with gpca_pkg.GpcaEngine() as e:
        e.upload_genotypes_i8(G)
        st = e.snp_stats(gpca_pkg.QcConfig(0.98, 0.01, 1.0))
        e.set_standardization(st["mu"], st["sigma"], st["keep"])
        rows = np.flatnonzero(st["keep"])
        K = len(rows)
        we = gio.ld_windows([fs.chromosomes[r] for r in rows], np.asarray(fs.positions, np.int64)[rows], "20kb")
        full = e.ld_score(we, partners=True)                                 # one call over all rows
        l2 = gpca_pkg.GpcaEngine.ld_score_total(full["score"])
        maf = gio.maf_from_qc_detail(*(e.snp_qc_detail()[0][rows][:, c] for c in (0, 2, 3)))
    assert miss[rows].any() and K < M                                        # missing calls among the rows, and the QC drops some
    lines = open(outs["py"] + ".l2.ldscore").read().split("\n")
    assert lines[0] == "CHR\tSNP\tBP\tL2" and lines[-1] == "" and len(lines) == K + 2
    for t, r in enumerate(rows):
        assert lines[1 + t] == f"{chrom[r]}\trs{r}\t{pos[r]}\t{'%.6g' % l2[t]}", (t, lines[1 + t])
    assert l2.mean() > 1.5 and full["partners"].max() <= 400
    assert open(outs["py"] + ".l2.M").read() == f"{K}\n" and open(outs["py"] + ".l2.M_5_50").read() == f"{int((maf > 0.05).sum())}\n"
    summ = open(outs["py"] + ".ldsc.summary").read().split("\n")
    assert summ[0].split("\t") == "#TRAIT TEST N M_USED MEAN_CHI2 LAMBDA_GC INTERCEPT INTERCEPT_SE H2 H2_SE RATIO RATIO_SE".split()
    assert [s.split("\t")[:2] for s in summ[1:3]] == [["height", "LINEAR"], ["case", "LOGISTIC"]] and summ[3:] == [""]
    for s in summ[1:3]:
        f = s.split("\t")
        assert f[2] == str(N - 6) and 0 < int(f[3]) <= K and all(v != "NA" for v in f[4:10])
