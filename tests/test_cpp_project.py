"""Both command lines on the projection path: fit a synthetic .bed with --gpca-save-model through each (the model files must be
byte-identical and hold what the fit used), then project a second .bed -- other samples, shuffled variant order, swapped alleles,
absent SNPs, an allele-mismatched SNP, 5 % missing calls -- through both: byte-identical Q.projected.pca.tsv, scores equal to a numpy
projection computed from the model file."""
import os
import subprocess

import numpy as np
import pytest

from genomic_pca_amd import io as gio
from genomic_pca_amd.cli import main

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "genomic_pca_amd", "bin", "genomic_pca")


@pytest.fixture(scope="module")
def host_bin():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "genomic_pca_amd", "host"), "-s"])
    return BIN


def _cohort(M, N, seed, p):
    rng = np.random.default_rng(seed)
    return (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)


def _native(host_bin, args):
    r = subprocess.run([host_bin, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


@pytest.mark.parametrize("local", [False, True])
def test_both_clis_save_and_project(tmp_path, host_bin, local):
    M, N, N2, k = 2000, 300, 211, 4
    rng = np.random.default_rng(15)
    p = rng.uniform(0.05, 0.5, size=(M, 1))
    G = _cohort(M, N, 16, p)
    ids = [f"rs{i}" for i in range(M)]
    pre = str(tmp_path / "fit")
    gio.write_plink(pre, G, [f"f{i}" for i in range(N)], ids, ["1"] * M, list(range(1, M + 1)))
    ld = tmp_path / "ld.txt"
    ld.write_text("1 1 1000\n1 1001 2000\n")
    fit = ["--eigensnp", "--bed-file", pre + ".bed", "--ld-block-file", str(ld), "--eigensnp-k-global", str(k),
           "--eigensnp-max-hwe-p", "1.0", "--gpca-save-model"]
    if local:
        fit += ["--gpca-eigensnp-local-stage", "--eigensnp-min-subset-size", "100"]
    out_py, out_c = str(tmp_path / "py" / "P"), str(tmp_path / "c" / "P")
    assert main(fit + ["--out", out_py]) == 0
    _native(host_bin, fit + ["--out", out_c])
    model_py = open(out_py + ".eigensnp.model.tsv", "rb").read()
    assert model_py == open(out_c + ".eigensnp.model.tsv", "rb").read()

    # the model holds what the fit used: the loadings file's rows (same order, '{:.6}'), the eigenvalues, the rows' mean / s.d.
    model = gio.read_model(out_py + ".eigensnp.model.tsv")
    lrows = [l.split("\t") for l in open(out_py + ".eigensnp.loadings.tsv").read().splitlines()[1:]]
    assert [r[0] for r in lrows] == model.variant_ids and [int(r[2]) for r in lrows] == model.positions
    assert all(f"{v:.6f}" == s for r, w in zip(lrows, model.loadings) for v, s in zip(w, r[3:]))
    ev = [l.split("\t")[1] for l in open(out_py + ".eigenvalues.tsv").read().splitlines()[1:]]
    assert [f"{v:.6f}" for v in model.eigenvalues] == ev
    rows = np.array([ids.index(v) for v in model.variant_ids])
    Gr = G[rows].astype(np.float64)
    mean, sd = Gr.mean(axis=1), Gr.std(axis=1, ddof=1)
    assert np.max(np.abs(model.mean - mean)) < 1e-5 and np.max(np.abs(model.sd / sd - 1)) < 1e-5
    assert model.n_samples == N and model.k == k and model.allele1[0] == "A" and model.allele2[0] == "G"

    # the target
    G2 = _cohort(M, N2, 17, p)
    order = rng.permutation(M)[: M - 30]
    T = G2[order].copy()
    tids = [ids[i] for i in order]
    alleles = [("A", "G")] * len(order)
    swap = set(rng.choice(len(order), 40, replace=False).tolist())
    for j in swap:
        alleles[j] = ("G", "A")
        T[j] = 2 - T[j]
    mism = min(set(range(len(order))) - swap)
    alleles[mism] = ("A", "C")
    T[rng.random(T.shape) < 0.05] = -127
    tpre = str(tmp_path / "target")
    gio.write_plink(tpre, T, [f"t{i}" for i in range(N2)], tids, ["1"] * len(order), list(range(len(order))), alleles=alleles)
    q_py, q_c = str(tmp_path / "py" / "Q"), str(tmp_path / "c" / "Q")
    assert main(["--gpca-project-model", out_py + ".eigensnp.model.tsv", "--bed-file", tpre + ".bed", "--out", q_py]) == 0
    r = _native(host_bin, ["--gpca-project-model", out_c + ".eigensnp.model.tsv", "--bed-file", tpre + ".bed", "--out", q_c])
    assert "matched" in r.stderr
    text = open(q_py + ".projected.pca.tsv", "rb").read()
    assert text == open(q_c + ".projected.pca.tsv", "rb").read()

    lines = text.decode().splitlines()
    assert lines[0].split("\t") == ["SampleID"] + [f"PC{i}" for i in range(1, k + 1)] + ["SNPsUsed"]
    body = [l.split("\t") for l in lines[1:]]
    assert [b[0] for b in body] == [f"t{i}" for i in range(N2)]
    sc = np.array([[float(v) for v in b[1:-1]] for b in body]); used = np.array([int(b[-1]) for b in body])
    pos = {v: s for s, v in enumerate(model.variant_ids)}
    ref = np.zeros((N2, k)); ref_used = np.zeros(N2, np.int64)
    for j, v in enumerate(tids):
        s = pos.get(v)
        if s is None or j == mism or not np.any(model.loadings[s]):
            continue
        g = T[j].astype(np.float64)
        mu, sdv, w = float(model.mean[s]), float(model.sd[s]), model.loadings[s].astype(np.float64)
        if j in swap:
            mu, w = 2.0 - mu, -w
        o = g != -127
        ref += np.outer(np.where(o, (g - mu) / sdv, 0.0), w)
        ref_used += o
    assert np.array_equal(used, ref_used)
    assert np.max(np.abs(sc - ref)) <= 1e-4 * np.max(np.abs(ref)) + 1e-6
