"""Both command lines with --gpca-sample-missing, --gpca-het, --gpca-mind and --gpca-het-sd, on a synthetic .bed of one population (160
samples, 1 000 SNPs, 20 SNPs that the call-rate filter drops and 200 that no LD block holds) with one quantitative trait.  Sample 10 is
contaminated (mixed 50/50 with sample 11), sample 50 has excess homozygosity, samples 5 and 120 miss 40 % of their calls on the SNPs
outside the LD blocks (the PCA itself takes no missing call on its own SNPs); sample 31 is a duplicate of sample 30 and sample 5 one of
sample 6.
The two programs write byte-identical P.smiss, P.het and P.sampleqc.in.id / .out.id; the files equal what the io writers produce from a
numpy model's counts over the SNPs that pass the SNP QC; with --gpca-king-cutoff the pair (5, 6) is dropped before the greedy rule
because 5 fails --gpca-mind, so 6 stays in the fit, while of (30, 31) the later one leaves; the scan's OBS_CT shows the smaller
include set; and with --gpca-sample-missing --gpca-het alone every other output file is byte-identical to a run without the flags.
CPU-only: the refusals, alike in both programs."""
import os
import subprocess

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import io as gio
from genomic_pca_amd.cli import main
from test_cpp_assoc_score import BIN, ROOT, gio_qc, host_bin  # noqa: F401  (fixtures)
from test_sample_qc_host import counts_model

M, N = 1000, 160
CONTAMINATED, HOMOZYGOUS, SPARSE, TWIN = 10, 50, [5, 120], 31
NEW = (".smiss", ".het", ".sampleqc.in.id", ".sampleqc.out.id")


@pytest.fixture(scope="module")
def fileset(tmp_path_factory):
    d = tmp_path_factory.mktemp("sample_qc")
    rng = np.random.default_rng(5)
    p = rng.uniform(0.1, 0.9, M)[:, None]
    G = (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)
    G[:, TWIN] = G[:, 30]
    G[:, 5] = G[:, 6]
    G[:, CONTAMINATED] = np.where(G[:, CONTAMINATED] != G[:, 11], 1, G[:, CONTAMINATED])
    flip = (G[:, HOMOZYGOUS] == 1) & (rng.random(M) < 0.4)
    G[flip, HOMOZYGOUS] = np.where(rng.random(int(flip.sum())) < 0.5, 0, 2)
    out_of_blocks = np.r_[400:500, 900:1000]                          # (these rows pass the QC, no LD block holds them)
    miss = rng.random((200, N)) < 0.003
    for n in SPARSE:
        miss[:, n] = rng.random(200) < 0.4
    G[out_of_blocks] = np.where(miss, -127, G[out_of_blocks])
    G[300:320][rng.random((20, N)) < 0.1] = -127                      # dropped by the call-rate filter
    pre = str(d / "in")
    gio.write_plink(pre, G, [f"s{i}" for i in range(N)], [f"rs{i}" for i in range(M)], ["1"] * M, list(range(1, M + 1)))
    with open(pre + ".fam", "w") as f:
        f.writelines(f"fam{i // 4}\ts{i}\t0\t0\t0\t-9\n" for i in range(N))
    ld = d / "ld.txt"
    ld.write_text("1 1 400\n1 501 900\n")
    with open(d / "y.pheno", "w") as f:
        f.write("FID IID height\n")
        f.writelines(f"fam{i // 4} s{i} {rng.normal():.6f}\n" for i in range(N))
    return pre, str(ld), str(d), G


def expected_files(tmp, fs, st, G, mind, het_sd):
    """the files from the numpy model's counts, through the io writers; returns (prefix, pass)"""
    rows = np.flatnonzero(st["keep"])
    counts, qc = counts_model(G[rows])
    q = gpca.het_weights(qc)
    qsum = (G[rows] != -127).T.astype(np.uint64) @ q.astype(np.uint64)
    het = gpca.sample_het(counts, qsum)
    pre = os.path.join(tmp, "want", "P")
    gio.write_smiss(pre, fs.family_ids, fs.sample_ids, counts, len(rows))
    gio.write_het(pre, fs.family_ids, fs.sample_ids, counts, het)
    ok = None
    if mind is not None or het_sd is not None:
        ok, why = gio.sample_qc_pass(counts, len(rows), het[:, 2], mind, het_sd)
        gio.write_sample_qc_ids(pre, fs.family_ids, fs.sample_ids, ok, why)
    return pre, ok


@pytest.mark.gpu
def test_both_clis_sample_qc(tmp_path, host_bin, fileset):
    from genomic_pca_amd import _lib
    from genomic_pca_amd.engine import GpcaEngine
    pre, ld, d, G = fileset
    fs = gio.read_plink(pre + ".bed")
    with GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=_lib.STORE_INT8) as eng:
        eng.upload_bed2bit(fs.bed_rows, fs.n_samples)
        st = eng.snp_stats(gio_qc())
    n_keep = int(st["keep"].sum())
    assert 800 < n_keep < M and not st["keep"][300:320].any() and st["keep"][900:].any()
    args = ["--eigensnp", "--bed-file", pre + ".bed", "--ld-block-file", ld, "--eigensnp-k-global", "3", "--eigensnp-max-hwe-p", "1.0",
            "--gpca-assoc-pcs", "2", "--gpca-assoc-pheno", os.path.join(d, "y.pheno"), "--gpca-king-cutoff", "0.177"]
    rep = ["--gpca-sample-missing", "--gpca-het"]
    full = rep + ["--gpca-mind", "0.05", "--gpca-het-sd", "3"]
    out = {n: str(tmp_path / n / "P") for n in ("py_full", "c_full", "py_rep", "c_rep", "plain")}
    assert main(args + full + ["--out", out["py_full"]]) == 0
    assert main(args + rep + ["--out", out["py_rep"]]) == 0
    for extra, name in ((full, "c_full"), (rep, "c_rep"), ([], "plain")):
        r = subprocess.run([host_bin, *args, *extra, "--out", out[name]], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
    files = lambda o: sorted(os.listdir(os.path.dirname(o)))
    read = lambda o, s: open(o + s, "rb").read()
    old = files(out["plain"])
    assert len(old) >= 5 and not any(f.endswith(NEW) for f in old)
    # the reports alone: two new files, everything else what the run without the flags writes
    want, _ = expected_files(str(tmp_path / "rep"), fs, st, G, None, None)
    for o in (out["py_rep"], out["c_rep"]):
        assert files(o) == sorted(old + ["P" + s for s in NEW[:2]])
        for s in NEW[:2]:
            assert read(o, s) == read(want, s) and len(read(o, s)) > 100, (o, s)
        for f in old:
            assert open(os.path.join(os.path.dirname(o), f), "rb").read() == open(os.path.join(os.path.dirname(out["plain"]), f), "rb").read(), (f, o)
    # the filters: the model flags the four samples that were made bad, and both programs write the model's files
    want, ok = expected_files(str(tmp_path / "full"), fs, st, G, 0.05, 3.0)
    assert sorted(np.flatnonzero(ok == 0).tolist()) == sorted(SPARSE + [CONTAMINATED, HOMOZYGOUS])
    for o in (out["py_full"], out["c_full"]):
        assert files(o) == sorted(old + ["P" + s for s in NEW])
        for s in NEW:
            assert read(o, s) == read(want, s), (o, s)
    assert read(out["py_full"], ".sampleqc.out.id").decode().split("\n")[:3] == ["#FID\tIID\tREASON", "fam1\ts5\tMIND", "fam2\ts10\tHET"]
    for f in old:                                             # (the two programs agree on every file of the filtered run too)
        assert open(os.path.join(os.path.dirname(out["py_full"]), f), "rb").read() == open(os.path.join(os.path.dirname(out["c_full"]), f), "rb").read(), f
    # KING: without the filters the pairs (5, 6) and (30, 31) each lose their later sample; with them the pair (5, 6) is dropped first
    king_out = lambda o: [ln.split("\t")[1] for ln in open(o + ".king.cutoff.out.id").read().split("\n")[1:-1]]
    # (the contaminated sample 10 shares no IBS0 site with its source 11: a pair of its own in the run without the filters)
    k_plain, k_full = king_out(out["plain"]), king_out(out["c_full"])
    assert "s6" in k_plain and "s31" in k_plain and k_full == king_out(out["py_full"])
    assert "s31" in k_full and "s6" not in k_full and not {"s5", "s10", "s11", "s50", "s120"} & set(k_full)
    # every sample is still scored; the scan's include set is KING's in-set and the pass mask
    assert len(open(out["c_full"] + ".eigensnp.pca.tsv").read().split("\n")) == len(open(out["plain"] + ".eigensnp.pca.tsv").read().split("\n")) == N + 2
    obs = lambda o: max(int(ln.split("\t")[4]) for ln in open(o + ".height.assoc.linear").read().split("\n")[1:-1])
    assert obs(out["plain"]) == N - len(k_plain) and obs(out["c_full"]) == obs(out["py_full"]) == N - 4 - len(k_full)


BASE = ["--bed-file", "t.bed", "--ld-block-file", "l.txt", "--out", "x"]
NEEDS_RESIDENT = ("--gpca-sample-missing, --gpca-het, --gpca-mind and --gpca-het-sd need the genotype matrix resident on the device: the "
                  "per-sample counts of a matrix walked out of core are not implemented")


def test_sample_qc_flag_refusals_are_the_same(tmp_path, host_bin):
    E = ["--eigensnp"]
    for flags, msg in ((["--gpca-het"], "--gpca-sample-missing, --gpca-het, --gpca-mind and --gpca-het-sd need the --eigensnp workflow"),
                       (["--gpca-mind", "0.1"], "--gpca-sample-missing, --gpca-het, --gpca-mind and --gpca-het-sd need the --eigensnp workflow"),
                       (E + ["--gpca-mind", "1"], "--gpca-mind must lie in [0, 1)"),
                       (E + ["--gpca-mind", "-0.1"], "--gpca-mind must lie in [0, 1)"),
                       (E + ["--gpca-mind", "nan"], "--gpca-mind must lie in [0, 1)"),
                       (E + ["--gpca-het-sd", "0"], "--gpca-het-sd must be finite and above 0"),
                       (E + ["--gpca-het-sd", "inf"], "--gpca-het-sd must be finite and above 0"),
                       (E + ["--gpca-het-sd", "3", "--gpca-eigensnp-local-stage"],
                        "--gpca-mind and --gpca-het-sd cannot be combined with --gpca-eigensnp-local-stage (that stage owns the sample mask)"),
                       (E + ["--gpca-sample-missing", "--gpca-stream", "on"], NEEDS_RESIDENT),
                       (E + ["--gpca-het-sd", "3", "--gpca-stream", "on"], NEEDS_RESIDENT)):
        with pytest.raises(SystemExit) as ei:
            main(BASE + flags)
        r = subprocess.run([host_bin, *BASE, *flags], capture_output=True, text=True, timeout=60)
        assert str(ei.value) == "error: " + msg, (flags, str(ei.value))
        assert r.returncode == 2 and r.stderr == "error: " + msg + "\n", (flags, r.stderr)
    # accepted values get as far as the missing fileset
    for ok in (["--gpca-sample-missing"], ["--gpca-het"], ["--gpca-mind", "0"], ["--gpca-het-sd", "2.5", "--gpca-mind", "0.02", "--gpca-het"],
               ["--gpca-sample-missing", "--gpca-eigensnp-local-stage"]):
        with pytest.raises(FileNotFoundError):
            main(BASE + E + ok)
    helptext = subprocess.run([host_bin, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert all(w in helptext for w in ("--gpca-sample-missing", "--gpca-het ", "--gpca-mind", "--gpca-het-sd"))
