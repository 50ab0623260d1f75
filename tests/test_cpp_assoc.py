"""Both command lines on the association path: --eigensnp --gpca-assoc-pheno on a synthetic .bed of two populations with planted
relatives, two traits and a covariate file, with and without --gpca-king-cutoff, write byte-identical P.<trait>.assoc.linear.  The scan
runs last, on the keep mask reset to the SNP QC: its files hold one row per SNP that passes the QC, the ones the LD blocks leave out of
the PCA included, and equal what GpcaEngine.assoc_linear gives for the traits, covariates and include mask the run handed it, on an
engine of the test's own that keeps the QC mask.  Missing calls sit only in rows the call-rate filter drops (the PCA takes fully called
SNPs only; the missing-call path of the scan is held to its bars in test_gpu_assoc.py).  The refusals carry the same text from both
programs."""
import os
import subprocess

import numpy as np
import pytest

from genomic_pca_amd import _lib
from genomic_pca_amd import io as gio
from genomic_pca_amd.cli import main
from genomic_pca_amd.engine import GpcaEngine, QcConfig
from test_assoc_host import BASE, NEEDS_RESIDENT, bad_flags, pheno_files
from test_cpp_pcrelate import cohort

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "genomic_pca_amd", "bin", "genomic_pca")
K_GLOBAL, PCS = 3, 2
CAUSAL = 1206           # a common SNP (A1 frequency 0.51) at position 1207, which no LD block holds: the PCA never sees it


@pytest.fixture(scope="module")
def host_bin():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "genomic_pca_amd", "host"), "-s"])
    return BIN


def test_flag_errors_cpp(tmp_path, host_bin):
    f = pheno_files(tmp_path)
    for flags, msg in bad_flags(f):
        r = subprocess.run([host_bin, *BASE, *flags], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stderr.startswith("error: ") and msg in r.stderr, (flags, r.stderr)
        with pytest.raises(SystemExit) as ei:                                          # the same text from the Python command line
            main(BASE + flags)
        assert str(ei.value) + "\n" == r.stderr
    assert "--gpca-assoc-pheno" in subprocess.run([host_bin, "--help"], capture_output=True, text=True, timeout=60).stdout


@pytest.fixture(scope="module")
def fileset(tmp_path_factory):
    d = tmp_path_factory.mktemp("assoc")
    rng = np.random.default_rng(41)
    G = cohort()
    M, N = G.shape
    G[300:320][rng.random((20, N)) < 0.1] = -127                      # dropped by the call-rate filter
    pre = str(d / "in")
    gio.write_plink(pre, G, [f"s{i}" for i in range(N)], [f"rs{i}" for i in range(M)], ["1"] * M, list(range(1, M + 1)))
    with open(pre + ".fam", "w") as f:
        f.writelines(f"fam{i // 4}\ts{i}\t0\t0\t0\t-9\n" for i in range(N))
    ld = d / "ld.txt"
    ld.write_text(f"1 1 1200\n1 1501 {M - 200}\n")                  # blocks that leave QC-passing SNPs out of the kept rows
    pop = (np.arange(N) >= 100) & (np.arange(N) < 200) | (np.arange(N) >= 205)
    y1 = 1.0 * pop + 1.0 * G[CAUSAL] + rng.standard_normal(N)
    y2 = rng.standard_normal(N)
    age = rng.uniform(20, 70, N)
    order = rng.permutation(N)
    with open(d / "traits.pheno", "w") as f:                          # shuffled rows; s3 absent; one NA; a sample the .fam does not have
        f.write("FID IID height bmi\nfam999 s999 1 2\n")
        for i in order:
            if i != 3:
                f.write(f"fam{i // 4} s{i} {float(y1[i])!r} {'NA' if i == 11 else repr(float(y2[i]))}\n")
    with open(d / "cov.txt", "w") as f:
        f.write("#FID\tIID\tage\n")
        f.writelines(f"fam{i // 4}\ts{i}\t{'nan' if i == 20 else repr(float(age[i]))}\n" for i in range(N))
    return pre, str(ld), str(d / "traits.pheno"), str(d / "cov.txt"), M, N


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [["--gpca-king-cutoff", "0.0884"], ["--gpca-assoc-vif", "20"]], ids=["inset", "everyone"])
def test_both_clis_assoc(tmp_path, host_bin, fileset, monkeypatch, extra):
    pre, ld, pheno, cov, M, N = fileset
    args = ["--eigensnp", "--bed-file", pre + ".bed", "--ld-block-file", ld, "--eigensnp-k-global", str(K_GLOBAL), "--eigensnp-max-hwe-p", "1.0",
            "--gpca-assoc-pheno", pheno, "--gpca-assoc-covar", cov, "--gpca-assoc-pcs", str(PCS), *extra]
    seen = []
    real = GpcaEngine.assoc_linear

    def spy(self, Y, covar=None, include=None, max_vif=50.0, rows=None, xb=False):
        seen.append((np.array(Y), np.array(covar), np.array(include, bool), max_vif, rows, self.num_pca_snps()))
        return real(self, Y, covar, include, max_vif, rows, xb)
    monkeypatch.setattr(GpcaEngine, "assoc_linear", spy)
    out_py, out_c = str(tmp_path / "py" / "P"), str(tmp_path / "c" / "P")
    assert main(args + ["--out", out_py]) == 0
    monkeypatch.undo()
    r = subprocess.run([host_bin, *args, "--out", out_c], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for ext in (".height.assoc.linear", ".bmi.assoc.linear", ".eigensnp.pca.tsv", ".eigensnp.loadings.tsv"):
        assert open(out_py + ext, "rb").read() == open(out_c + ext, "rb").read(), ext
    assert "association scan of" in r.stderr

    # what the run handed gpca_assoc_linear: both traits, the first PCS columns of the scores it wrote and the covariate, the samples
    # with everything present (and in the in-set), on the keep mask of the SNP QC
    inset_run = extra[0] == "--gpca-king-cutoff"
    assert len(seen) == 1                                                              # one band at this size
    Y, C, inc, vif, rows, k_scan = seen[0]
    sc = np.loadtxt(out_py + ".eigensnp.pca.tsv", skiprows=1, usecols=range(1, 1 + PCS))
    assert Y.shape == (N, 2) and C.shape == (N, PCS + 1) and np.all(np.abs(C[:, :PCS] - sc) <= 0.5e-6 + 1e-12 * np.abs(sc))
    assert vif == (50.0 if inset_run else 20.0)
    iids = [f"s{i}" for i in range(N)]
    want_inc = np.ones(N, bool)
    want_inc[[3, 11, 20]] = False
    assert np.isnan(Y[3]).all() and np.isnan(Y[11, 1]) and np.isnan(C[20, PCS])
    if inset_run:
        ins = {ln.split("\t")[1] for ln in open(out_py + ".king.cutoff.in.id").read().split("\n")[1:-1]}
        in_mask = np.array([s in ins for s in iids])
        assert 2 <= N - int(in_mask.sum()) <= 8
        want_inc &= in_mask
    assert np.array_equal(inc, want_inc)

    # the files against GpcaEngine.assoc_linear on an engine loaded here that keeps the QC mask: more rows than the PCA saw
    fs = gio.read_plink(pre + ".bed")
    with GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=_lib.STORE_INT8) as eng:
        eng.upload_bed2bit(fs.bed_rows, fs.n_samples)
        st = eng.snp_stats(QcConfig(0.98, 0.01, 1.0))
        keep, _ = gio.map_snps_to_ld_blocks(gio.parse_ld_block_file(ld), fs.chromosomes, fs.positions, st["keep"])
        n_qc, n_pca = int(st["keep"].sum()), int(keep.sum())
        assert 0 < n_pca < n_qc <= M - 20 and not st["keep"][300:320].any()
        counts, _ = eng.snp_qc_detail()
        eng.set_standardization(st["mu"], st["sigma"], st["keep"])
        res = eng.assoc_linear(Y, C, include=inc, max_vif=vif)
    assert rows == (0, n_qc) and k_scan == n_qc
    assert open(out_py + ".eigensnp.loadings.tsv").read().count("\n") == 1 + n_pca     # the PCA saw the block-mapped set only
    qc_rows = np.flatnonzero(st["keep"])
    maf = gio.maf_from_qc_detail(counts[:, 0], counts[:, 2], counts[:, 3])
    assert n_qc == int(((counts[:, 0] >= 0.98 * N) & (maf >= 0.01)).sum())             # the QC detail: call rate and MAF (HWE is off)
    df = int(inc.sum()) - (PCS + 1) - 2
    lib = _lib.load()
    want = str(tmp_path / "want")
    for t, name in enumerate(("height", "bmi")):
        lp = [lib.gpca_student_t_log10p(float(v), float(df)) if v == v else float("nan") for v in res["t"][:, t]]
        gio.write_assoc(want, name, [fs.chromosomes[i] for i in qc_rows], [fs.positions[i] for i in qc_rows], [fs.variant_ids[i] for i in qc_rows],
                        [fs.allele1[i] for i in qc_rows], res["n_obs"], res["a1_freq"], res["beta"][:, t], res["se"][:, t], res["t"][:, t], lp)
        assert open(f"{want}.{name}.assoc.linear", "rb").read() == open(f"{out_py}.{name}.assoc.linear", "rb").read(), name

    # the layout: one line per QC-passing SNP in .bed order, every included sample observed; the planted SNP is the top hit of its trait
    lines = open(out_py + ".height.assoc.linear").read().split("\n")
    assert lines[0] == "#CHROM\tPOS\tID\tA1\tOBS_CT\tA1_FREQ\tBETA\tSE\tT_STAT\tLOG10P" and lines[-1] == ""
    body = [ln.split("\t") for ln in lines[1:-1]]
    assert [b[2] for b in body] == [f"rs{i}" for i in qc_rows] and len(body) == n_qc
    assert {b[4] for b in body} == {str(int(inc.sum()))}
    outside = [b for b in body if 1200 < int(b[1]) <= 1500]
    assert outside and all(b[6] != "NA" for b in outside)                              # SNPs no LD block holds are tested
    lp = np.array([float(b[9]) if b[9] != "NA" else 0.0 for b in body])
    assert body[int(np.argmax(lp))][2] == f"rs{CAUSAL}" and 1200 < CAUSAL + 1 <= 1500 and lp.max() > 6


@pytest.mark.gpu
def test_refusals_carry_the_same_text(tmp_path, host_bin, fileset, monkeypatch):
    pre, ld, pheno, cov, M, N = fileset
    args = ["--eigensnp", "--bed-file", pre + ".bed", "--ld-block-file", ld, "--eigensnp-k-global", str(K_GLOBAL), "--eigensnp-max-hwe-p", "1.0",
            "--gpca-assoc-pheno", pheno, "--out", str(tmp_path / "P")]
    monkeypatch.setenv("GPCA_CLI_FREE_BYTES", str(1 << 20))                            # out of core: the matrix "does not fit"
    cases = [(["--gpca-stream", "on"], 2), (["--gpca-eigensnp-local-stage"], 2), ([], 1)]
    for extra, code in cases:
        r = subprocess.run([host_bin, *args, *extra], capture_output=True, text=True, timeout=300)
        with pytest.raises(SystemExit) as ei:
            main(args + extra)
        last = r.stderr.strip().split("\n")[-1]
        assert r.returncode == code and last == str(ei.value) and last.startswith("error: --gpca-assoc-pheno"), r.stderr
        if extra != ["--gpca-eigensnp-local-stage"]:
            assert NEEDS_RESIDENT in last
    assert not os.path.exists(str(tmp_path / "P") + ".height.assoc.linear")
