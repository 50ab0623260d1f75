"""Both command lines with --gpca-admixture-cv, on a synthetic .bed of 90 samples and 320 SNPs built here: two Balding-Nichols populations
(Fst 0.15) of 40 samples with admixed samples among them and ten duplicates (so --gpca-king-cutoff leaves mode-2 samples).  The two
programs write byte-identical P.admix.cv with --gpca-admixture 2 --gpca-admixture-cv 3 --gpca-admixture-cv-k 1-3, with and without
--gpca-king-cutoff; the file equals io.write_admix_cv of GpcaEngine.admix_cv under the keep mask and modes the command lines use; every
other file, the admixture fit's included, is byte-identical to a run without the CV flags.  CPU-only: the refusals, alike in both
programs."""
import os
import subprocess

import numpy as np
import pytest

from genomic_pca_amd import io as gio
from genomic_pca_amd.cli import main
from test_cpp_assoc_score import BIN, ROOT, gio_qc, host_bin  # noqa: F401  (fixtures)

M, N = 320, 90
FIT = ["--gpca-admixture", "2", "--gpca-admixture-seed", "5", "--gpca-admixture-tol", "1e-5"]
CV = ["--gpca-admixture-cv", "3", "--gpca-admixture-cv-seed", "9", "--gpca-admixture-cv-k", "1-3"]


@pytest.fixture(scope="module")
def fileset(tmp_path_factory):
    d = tmp_path_factory.mktemp("admixcv")
    rng = np.random.default_rng(41)
    fst, K = 0.15, 2
    p = rng.uniform(0.1, 0.9, M)
    F = np.clip(rng.beta(p[:, None] * (1 - fst) / fst, (1 - p[:, None]) * (1 - fst) / fst, (M, K)), 0.02, 0.98)
    Q = np.zeros((80, K))
    for k in range(K):
        Q[40 * k:40 * k + 30, k] = 1
        Q[40 * k + 30:40 * k + 40] = rng.dirichlet(np.full(K, 0.7), 10)
    P = F @ Q.T
    G = ((rng.random((M, 80)) < P).astype(np.int8) + (rng.random((M, 80)) < P).astype(np.int8))
    G = np.concatenate([G, G[:, 3:80:8]], 1)                            # ten duplicates
    pre = str(d / "in")
    gio.write_plink(pre, G, [f"s{i}" for i in range(N)], [f"rs{i}" for i in range(M)], ["1"] * M, list(range(1, M + 1)))
    ld = d / "ld.txt"
    ld.write_text("1 1 900000\n")
    return pre, str(ld)


def expected_cv(pre, out_py, king):
    """io.write_admix_cv of GpcaEngine.admix_cv under the keep mask and the modes the command lines use"""
    from genomic_pca_amd import _lib
    from genomic_pca_amd.engine import GpcaEngine
    fs = gio.read_plink(pre + ".bed")
    mode = None
    if king:
        inset = {tuple(ln.split()) for ln in open(out_py + ".king.cutoff.in.id") if not ln.startswith("#")}
        mode = np.array([0 if (f, i) in inset else 2 for f, i in zip(fs.family_ids, fs.sample_ids)], np.uint8)
    table = []
    with GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=_lib.STORE_INT8) as eng:
        eng.upload_bed2bit(fs.bed_rows, fs.n_samples)
        st = eng.snp_stats(gio_qc())
        keep = np.isin(np.array(fs.variant_ids), open(out_py + ".2.P.id").read().split()).astype(np.uint8)   # the SNPs the PCA was fitted on
        assert 0 < keep.sum() and not (keep & ~st["keep"].astype(np.uint8)).any()
        eng.set_standardization(st["mu"], st["sigma"], keep)
        for k in (1, 2, 3):
            cv = eng.admix_cv(k, folds=3, cv_seed=9, seed=5, tol=1e-5, mode=mode)
            table += [dict(K=k, folds=3, cv_seed=9, fold=c, **f) for c, f in enumerate(cv["folds"])]
    return table, mode


@pytest.mark.gpu
@pytest.mark.parametrize("king", [False, True], ids=["all samples", "king cutoff"])
def test_both_clis_admixture_cv(tmp_path, host_bin, fileset, king):
    pre, ld = fileset
    args = ["--eigensnp", "--bed-file", pre + ".bed", "--ld-block-file", ld, "--eigensnp-k-global", "2", "--eigensnp-max-hwe-p", "1.0"]
    if king:
        args += ["--gpca-king-cutoff", "0.3"]
    out = {n: str(tmp_path / n / "P") for n in ("py", "c", "plain")}
    assert main(args + FIT + CV + ["--out", out["py"]]) == 0
    logs = {}
    for extra, name in ((FIT + CV, "c"), (FIT, "plain")):
        r = subprocess.run([host_bin, *args, *extra, "--out", out[name]], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        logs[name] = r.stderr
    files = lambda o: sorted(os.listdir(os.path.dirname(o)))
    old = files(out["plain"])
    assert "P.2.Q" in old and "P.admix.cv" not in old and "CV error" not in logs["plain"]
    table, mode = expected_cv(pre, out["py"], king)
    if king:
        assert int((mode == 2).sum()) == 10
    want = gio.write_admix_cv(str(tmp_path / "want"), table)
    text = open(want).read()
    for o in (out["py"], out["c"]):
        assert files(o) == sorted(old + ["P.admix.cv"])                                  # no Q or P file of another K
        assert open(o + ".admix.cv").read() == text, o
        for f in old:                                                                    # the CV changes no other byte
            assert open(os.path.join(os.path.dirname(o), f), "rb").read() == open(os.path.join(os.path.dirname(out["plain"]), f), "rb").read(), (f, o)
    lines = [ln.split("\t") for ln in text.splitlines()]
    assert lines[0] == ["#K", "FOLDS", "CV_SEED", "FOLD", "STEPS", "CONVERGED", "N_HELD", "DEVIANCE", "CV_ERROR"] and len(lines) == 1 + 3 * 4
    assert [ln[0] for ln in lines[1:]] == ["1"] * 4 + ["2"] * 4 + ["3"] * 4 and [ln[3] for ln in lines[1:5]] == ["0", "1", "2", "*"]
    total = {int(ln[0]): ln for ln in lines[1:] if ln[3] == "*"}
    n_rows = len(open(out["c"] + ".2.P.id").read().split())
    assert all(int(t[6]) == n_rows * N for t in total.values())                          # every call is held exactly once (none is missing)
    assert float(total[2][8]) < float(total[1][8])                                       # two populations: K = 2 beats K = 1
    for k, t in total.items():
        assert f"CV error (K={k}): {t[8]}" in logs["c"], (k, logs["c"])


BASE = ["--bed-file", "t.bed", "--ld-block-file", "l.txt", "--out", "x"]
NEEDS_FIT = "--gpca-admixture-cv, --gpca-admixture-cv-seed and --gpca-admixture-cv-k need --gpca-admixture"
NEEDS_CV = "--gpca-admixture-cv-seed and --gpca-admixture-cv-k need --gpca-admixture-cv"
BAD_RANGE = "--gpca-admixture-cv-k must be A-B with 1 <= A <= B <= 16"
NEEDS_RESIDENT = "--gpca-admixture needs the genotype matrix resident on the device: the fit of a matrix walked out of core is not implemented"


def test_cv_flag_refusals_are_the_same(tmp_path, host_bin):
    E = ["--eigensnp"]
    A = E + ["--gpca-admixture", "3"]
    C = A + ["--gpca-admixture-cv"]
    w3 = tmp_path / "w3.txt"
    w3.write_text("FID IID GROUP\nf s1 a\nf s2 b\nf s3 c\n")
    sup = ["--gpca-admixture-supervised", "--gpca-within", str(w3)]
    for flags, msg in ((E + ["--gpca-admixture-cv"], NEEDS_FIT), (E + ["--gpca-admixture-cv", "4"], NEEDS_FIT),
                       (E + ["--gpca-admixture-cv-seed", "1"], NEEDS_FIT), (E + ["--gpca-admixture-cv-k", "1-3"], NEEDS_FIT),
                       (A + ["--gpca-admixture-cv-seed", "1"], NEEDS_CV), (A + ["--gpca-admixture-cv-k", "1-3"], NEEDS_CV),
                       (["--gpca-admixture", "3", "--gpca-admixture-cv"], "--gpca-admixture needs the --eigensnp workflow"),
                       (A + ["--gpca-admixture-cv", "1"], "--gpca-admixture-cv V must lie in [2, 64]"),
                       (A + ["--gpca-admixture-cv", "65"], "--gpca-admixture-cv V must lie in [2, 64]"),
                       (A + ["--gpca-admixture-cv", "-3"], "--gpca-admixture-cv V must lie in [2, 64]"),
                       (A + ["--gpca-admixture-cv=0"], "--gpca-admixture-cv V must lie in [2, 64]"),
                       (C + ["--gpca-admixture-cv-seed", "-1"], "--gpca-admixture-cv-seed must lie in [0, 2^63)"),
                       (C + ["--gpca-admixture-cv-k", "0-3"], BAD_RANGE), (C + ["--gpca-admixture-cv-k", "3-2"], BAD_RANGE),
                       (C + ["--gpca-admixture-cv-k", "1-17"], BAD_RANGE), (C + ["--gpca-admixture-cv-k", "3"], BAD_RANGE),
                       (C + ["--gpca-admixture-cv-k", "1-2-3"], BAD_RANGE), (C + ["--gpca-admixture-cv-k", "a-b"], BAD_RANGE),
                       (C + ["--gpca-admixture-cv-k=-3"], BAD_RANGE), (C + ["--gpca-admixture-cv-k", "1-"], BAD_RANGE),
                       (C + sup + ["--gpca-admixture-cv-k", "1-3"],
                        "--gpca-admixture-cv-k cannot be combined with --gpca-admixture-supervised (the groups fix K)"),
                       (C + ["--gpca-eigensnp-local-stage"],
                        "--gpca-admixture cannot be combined with --gpca-eigensnp-local-stage (that stage owns the sample mask and the keep mask)"),
                       (C + ["--gpca-stream", "on"], NEEDS_RESIDENT), (C + ["--gpca-admixture-cv-k", "1-3", "--gpca-stream", "on"], NEEDS_RESIDENT)):
        with pytest.raises(SystemExit) as ei:
            main(BASE + flags)
        r = subprocess.run([host_bin, *BASE, *flags], capture_output=True, text=True, timeout=60)
        assert str(ei.value) == "error: " + msg, (flags, str(ei.value))
        assert r.returncode == 2 and r.stderr == "error: " + msg + "\n", (flags, r.stderr)
    # accepted values get as far as the missing fileset
    for ok in (["--gpca-admixture-cv"], ["--gpca-admixture-cv", "2"], ["--gpca-admixture-cv", "64", "--gpca-admixture-cv-seed", "9223372036854775807"],
               ["--gpca-admixture-cv", "--gpca-admixture-cv-k", "1-16"], ["--gpca-admixture-cv=7", "--gpca-admixture-cv-k", "05-05"],
               ["--gpca-admixture-cv"] + sup):
        with pytest.raises(FileNotFoundError):
            main(BASE + A + ok)
        r = subprocess.run([host_bin, *BASE, *A, *ok], capture_output=True, text=True, timeout=60)
        assert r.returncode != 2 and "t.fam" in r.stderr, (ok, r.stderr)
    helptext = subprocess.run([host_bin, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert all(w in helptext for w in ("--gpca-admixture-cv [V]", "--gpca-admixture-cv-seed", "--gpca-admixture-cv-k"))
