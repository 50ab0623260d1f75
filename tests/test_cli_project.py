"""End to end through the Python CLI: fit a synthetic .bed with --gpca-save-model (global and local-stage EigenSNP), project a
second .bed (other samples, shuffled variant order, swapped alleles, absent SNPs, an allele-mismatched SNP, 5 % missing calls)
with --gpca-project-model, and check the scores against a numpy projection computed from the model file."""
import numpy as np
import pytest

from genomic_pca_amd import io as gio
from genomic_pca_amd.cli import main

pytestmark = pytest.mark.gpu


def _cohort(M, N, seed, p):
    rng = np.random.default_rng(seed)
    return ((rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8))


def _read_projected(path):
    lines = open(path).read().splitlines()
    hdr = lines[0].split("\t")
    rows = [l.split("\t") for l in lines[1:]]
    return hdr, [r[0] for r in rows], np.array([[float(v) for v in r[1:-1]] for r in rows]), np.array([int(r[-1]) for r in rows])


@pytest.mark.parametrize("local", [False, True])
def test_fit_save_model_then_project(tmp_path, local):
    M, N, N2, k = 2000, 300, 211, 4
    rng = np.random.default_rng(5)
    p = rng.uniform(0.05, 0.5, size=(M, 1))
    G = _cohort(M, N, 6, p)
    ids = [f"rs{i}" for i in range(M)]
    pre = str(tmp_path / "fit")
    gio.write_plink(pre, G, [f"f{i}" for i in range(N)], ids, ["1"] * M, list(range(1, M + 1)))
    ld = tmp_path / "ld.txt"
    ld.write_text("1 1 1000\n1 1001 2000\n")
    out = str(tmp_path / "P")
    args = ["--eigensnp", "--bed-file", pre + ".bed", "--ld-block-file", str(ld), "--out", out, "--eigensnp-k-global", str(k),
            "--eigensnp-max-hwe-p", "1.0", "--gpca-save-model"]
    if local:
        args += ["--gpca-eigensnp-local-stage", "--eigensnp-min-subset-size", "100"]
    assert main(args) == 0
    model = gio.read_model(out + ".eigensnp.model.tsv")
    assert model.k == k and model.n_samples == N and len(model.variant_ids) > 1500
    ev = [float(l.split("\t")[1]) for l in open(out + ".eigenvalues.tsv").read().splitlines()[1:]]
    assert np.allclose(model.eigenvalues, ev, rtol=1e-5)

    # the target: other samples, variants shuffled, 30 absent, 40 with swapped alleles (dosages of the other allele), one with a
    # different allele pair, 5 % missing calls
    G2 = _cohort(M, N2, 7, p)
    order = rng.permutation(M)[: M - 30]
    T = G2[order].copy()
    tids = [ids[i] for i in order]
    alleles = [("A", "G")] * len(order)
    swap = rng.choice(len(order), 40, replace=False)
    for j in swap:
        alleles[j] = ("G", "A")
        T[j] = 2 - T[j]
    mism = int(np.setdiff1d(np.arange(len(order)), swap)[0])
    alleles[mism] = ("A", "C")
    T[rng.random(T.shape) < 0.05] = -127
    tpre = str(tmp_path / "target")
    gio.write_plink(tpre, T, [f"t{i}" for i in range(N2)], tids, ["1"] * len(order), list(range(len(order))), alleles=alleles)
    q = str(tmp_path / "Q")
    assert main(["--gpca-project-model", out + ".eigensnp.model.tsv", "--bed-file", tpre + ".bed", "--out", q]) == 0
    hdr, names, sc, used = _read_projected(q + ".projected.pca.tsv")
    assert hdr == ["SampleID"] + [f"PC{i}" for i in range(1, k + 1)] + ["SNPsUsed"] and names == [f"t{i}" for i in range(N2)]

    # numpy from the model file: align by hand, mean-impute, project
    pos = {v: s for s, v in enumerate(model.variant_ids)}
    ref = np.zeros((N2, k)); ref_used = np.zeros(N2, np.int64)
    for j, v in enumerate(tids):
        s = pos.get(v)
        if s is None or j == mism or not np.any(model.loadings[s]):
            continue
        g = T[j].astype(np.float64)
        mu, sd, w = float(model.mean[s]), float(model.sd[s]), model.loadings[s].astype(np.float64)
        if j in set(swap.tolist()):
            mu, w = 2.0 - mu, -w
        obs = g != -127
        ref += np.outer(np.where(obs, (g - mu) / sd, 0.0), w)
        ref_used += obs
    assert np.array_equal(used, ref_used)
    assert np.max(np.abs(sc - ref)) <= 1e-4 * np.max(np.abs(ref)) + 1e-6
