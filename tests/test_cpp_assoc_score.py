"""Both command lines with --gpca-assoc-logistic: --eigensnp --gpca-assoc-pheno on the synthetic .bed of tests/test_cpp_assoc.py (two
populations with planted relatives), one case / control trait and one quantitative trait, --gpca-king-cutoff and a covariate file.
The two programs write byte-identical P.cad.assoc.logistic and P.height.assoc.linear; the linear file is the same with and without
the flag (without it the case / control column is one more trait of the linear scan, which moves no bit of another trait's column); a
1 / 2-coded and a 0 / 1-coded copy of the trait give the same file; the logistic file equals what GpcaEngine.assoc_logistic_score gives
for the trait, covariates and include mask the run handed it; a trait whose null model cannot be fitted stops both programs with its
name before any file of it is written."""
import os
import subprocess

import numpy as np
import pytest

from genomic_pca_amd import _lib
from genomic_pca_amd import io as gio
from genomic_pca_amd.cli import main
from genomic_pca_amd.engine import GpcaEngine
from test_cpp_pcrelate import cohort

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "genomic_pca_amd", "bin", "genomic_pca")
K_GLOBAL, PCS = 3, 2
CAUSAL = 1206           # a common SNP at position 1207, which no LD block holds (tests/test_cpp_assoc.py)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host_bin():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "genomic_pca_amd", "host"), "-s"])
    return BIN


@pytest.fixture(scope="module")
def fileset(tmp_path_factory):
    d = tmp_path_factory.mktemp("assoc_score")
    rng = np.random.default_rng(43)
    G = cohort()
    M, N = G.shape
    G[300:320][rng.random((20, N)) < 0.1] = -127                      # dropped by the call-rate filter
    pre = str(d / "in")
    gio.write_plink(pre, G, [f"s{i}" for i in range(N)], [f"rs{i}" for i in range(M)], ["1"] * M, list(range(1, M + 1)))
    with open(pre + ".fam", "w") as f:
        f.writelines(f"fam{i // 4}\ts{i}\t0\t0\t0\t-9\n" for i in range(N))
    ld = d / "ld.txt"
    ld.write_text(f"1 1 1200\n1 1501 {M - 200}\n")
    pop = (np.arange(N) >= 100) & (np.arange(N) < 200) | (np.arange(N) >= 205)
    eta = -0.8 + 1.0 * pop + 1.2 * (G[CAUSAL] - G[CAUSAL].mean())
    cc = (rng.random(N) < 1.0 / (1.0 + np.exp(-eta))).astype(int)
    height = 1.0 * pop + 1.0 * G[CAUSAL] + rng.standard_normal(N)
    age = rng.uniform(20, 70, N)
    order = rng.permutation(N)
    for name, shift in (("t12", 1), ("t01", 0)):                      # plink's 1 / 2 coding and the 0 / 1 coding of the same trait
        with open(d / f"{name}.pheno", "w") as f:                     # shuffled rows; s3 absent; one NA; a sample the .fam does not have
            f.write(f"FID IID cad height\nfam999 s999 {shift} 2\n")
            for i in order:
                if i != 3:
                    f.write(f"fam{i // 4} s{i} {'NA' if i == 11 else cc[i] + shift} {float(height[i])!r}\n")
    with open(d / "sep.pheno", "w") as f:                             # a case / control trait that the covariate separates
        f.write("FID IID sep height\n")
        f.writelines(f"fam{i // 4} s{i} {int(age[i] > 45)} {float(height[i])!r}\n" for i in range(N))
    with open(d / "cov.txt", "w") as f:
        f.write("#FID\tIID\tage\n")
        f.writelines(f"fam{i // 4}\ts{i}\t{'nan' if i == 20 else repr(float(age[i]))}\n" for i in range(N))
    return pre, str(ld), str(d), str(d / "cov.txt"), M, N


def test_both_clis_assoc_logistic(tmp_path, host_bin, fileset, monkeypatch):
    pre, ld, d, cov, M, N = fileset
    base = ["--eigensnp", "--bed-file", pre + ".bed", "--ld-block-file", ld, "--eigensnp-k-global", str(K_GLOBAL), "--eigensnp-max-hwe-p", "1.0",
            "--gpca-assoc-covar", cov, "--gpca-assoc-pcs", str(PCS), "--gpca-king-cutoff", "0.0884"]
    args = base + ["--gpca-assoc-pheno", os.path.join(d, "t12.pheno")]
    seen = []
    real = GpcaEngine.assoc_logistic_score

    def spy(self, Y, covar=None, include=None, max_vif=50.0, rows=None, ua=False):
        seen.append((np.array(Y), np.array(covar), np.array(include, bool), max_vif, rows, self.num_pca_snps()))
        return real(self, Y, covar, include, max_vif, rows, ua)
    monkeypatch.setattr(GpcaEngine, "assoc_logistic_score", spy)
    out_py, out_c, out_01, out_lin = (str(tmp_path / n / "P") for n in ("py", "c", "c01", "lin"))
    assert main(args + ["--gpca-assoc-logistic", "--out", out_py]) == 0
    monkeypatch.undo()
    r = subprocess.run([host_bin, *args, "--gpca-assoc-logistic", "--out", out_c], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "logistic score scan of" in r.stderr and "association scan of" in r.stderr
    for ext in (".cad.assoc.logistic", ".height.assoc.linear", ".eigensnp.pca.tsv"):
        assert open(out_py + ext, "rb").read() == open(out_c + ext, "rb").read(), ext
    assert not os.path.exists(out_py + ".cad.assoc.linear") and not os.path.exists(out_c + ".cad.assoc.linear")
    # the 0 / 1-coded copy of the trait: the same files
    r = subprocess.run([host_bin, *base, "--gpca-assoc-pheno", os.path.join(d, "t01.pheno"), "--gpca-assoc-logistic", "--out", out_01],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for ext in (".cad.assoc.logistic", ".height.assoc.linear"):
        assert open(out_01 + ext, "rb").read() == open(out_c + ext, "rb").read(), ext
    # without the flag: the linear file of the quantitative trait does not move, and the case / control column is a linear trait
    r = subprocess.run([host_bin, *args, "--out", out_lin], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert open(out_lin + ".height.assoc.linear", "rb").read() == open(out_c + ".height.assoc.linear", "rb").read()
    assert os.path.exists(out_lin + ".cad.assoc.linear") and not os.path.exists(out_lin + ".cad.assoc.logistic")

    # what the run handed gpca_assoc_logistic_score, and the file against a call of the test's own on the QC mask
    assert len(seen) == 1
    Y, C, inc, vif, rows, k_scan = seen[0]
    assert Y.shape == (N, 1) and C.shape == (N, PCS + 1) and vif == 50.0 and set(np.unique(Y[inc])) == {0.0, 1.0}
    assert not inc[3] and not inc[11] and not inc[20] and 2 <= N - int(inc.sum()) - 3 <= 8          # absent, NA, nan, and the KING out-set
    fs = gio.read_plink(pre + ".bed")
    with GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=_lib.STORE_INT8) as eng:
        eng.upload_bed2bit(fs.bed_rows, fs.n_samples)
        st = eng.snp_stats(gio_qc())
        eng.set_standardization(st["mu"], st["sigma"], st["keep"])
        res = eng.assoc_logistic_score(Y, C, include=inc, max_vif=vif)
    qc_rows = np.flatnonzero(st["keep"])
    assert rows == (0, len(qc_rows)) and k_scan == len(qc_rows)
    lib = _lib.load()
    want = str(tmp_path / "want")
    lp = [lib.gpca_normal_log10p(float(v)) if v == v else float("nan") for v in res["z"][:, 0]]
    gio.write_assoc_logistic(want, "cad", [fs.chromosomes[i] for i in qc_rows], [fs.positions[i] for i in qc_rows], [fs.variant_ids[i] for i in qc_rows],
                             [fs.allele1[i] for i in qc_rows], res["n_obs"], res["a1_freq"], res["beta"][:, 0], res["se"][:, 0], res["z"][:, 0], lp)
    assert open(want + ".cad.assoc.logistic", "rb").read() == open(out_py + ".cad.assoc.logistic", "rb").read()
    lines = open(out_py + ".cad.assoc.logistic").read().split("\n")
    assert lines[0] == "#CHROM\tPOS\tID\tA1\tOBS_CT\tA1_FREQ\tBETA\tSE\tZ_STAT\tLOG10P" and lines[-1] == ""
    body = [ln.split("\t") for ln in lines[1:-1]]
    assert [b[2] for b in body] == [f"rs{i}" for i in qc_rows] and {b[4] for b in body} == {str(int(inc.sum()))}
    lpv = np.array([float(b[9]) if b[9] != "NA" else 0.0 for b in body])
    assert body[int(np.argmax(lpv))][2] == f"rs{CAUSAL}" and lpv.max() > 4             # the planted SNP is the top hit


def gio_qc():
    from genomic_pca_amd.engine import QcConfig
    return QcConfig(0.98, 0.01, 1.0)


def test_a_failed_null_fit_names_the_trait(tmp_path, host_bin, fileset):
    pre, ld, d, cov, M, N = fileset
    args = ["--eigensnp", "--bed-file", pre + ".bed", "--ld-block-file", ld, "--eigensnp-k-global", str(K_GLOBAL), "--eigensnp-max-hwe-p", "1.0",
            "--gpca-assoc-covar", cov, "--gpca-assoc-pcs", "0", "--gpca-assoc-pheno", os.path.join(d, "sep.pheno"), "--gpca-assoc-logistic",
            "--out", str(tmp_path / "P")]
    r = subprocess.run([host_bin, *args], capture_output=True, text=True, timeout=300)
    with pytest.raises(SystemExit) as ei:
        main(args)
    last = r.stderr.strip().split("\n")[-1]
    assert r.returncode == 1 and last == str(ei.value), r.stderr
    assert last.startswith("error: --gpca-assoc-logistic: trait sep: the null model cannot be fitted") and "converge" in last.lower()
    assert not os.path.exists(str(tmp_path / "P") + ".sep.assoc.logistic") and not os.path.exists(str(tmp_path / "P") + ".height.assoc.linear")
