"""Both command lines on the KING path: --eigensnp --gpca-make-king --gpca-king-cutoff on a synthetic .bed of two populations with
planted relatives write byte-identical P.kin0, cut-off id files and P.eigensnp.pca.tsv; the out-set is the greedy rule's pick from the
table; the relatives' scores are their projection onto the in-set's PCs (a --gpca-project-model run of the saved model agrees)."""
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


def cohort(M=3000, n_pop=100, F=0.2, seed=17):
    """two Balding-Nichols populations; per population a duplicate, and a family of two parents and two children"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, M)
    freqs = [rng.beta(p * (1 - F) / F, (1 - p) * (1 - F) / F) for _ in range(2)]
    cols = []

    def draw(f):
        return (rng.random(M) < f).astype(np.int8) + (rng.random(M) < f).astype(np.int8)

    def child(x, y):
        hx = np.where(x == 2, 1, np.where(x == 0, 0, rng.integers(0, 2, M)))
        hy = np.where(y == 2, 1, np.where(y == 0, 0, rng.integers(0, 2, M)))
        return (hx + hy).astype(np.int8)
    for k in range(2):
        cols += [draw(freqs[k]) for _ in range(n_pop)]
    for k in range(2):
        P1, P2 = draw(freqs[k]), draw(freqs[k])
        cols += [cols[k * n_pop + 5].copy(), P1, P2, child(P1, P2), child(P1, P2)]
    return np.stack(cols, axis=1)


# one block over every SNP, and blocks that leave QC-passing SNPs out (a gap between them, a tail after the last)
@pytest.mark.parametrize("blocks", [lambda M: f"1 1 {M}\n", lambda M: f"1 1 1200\n1 1501 {M - 200}\n"], ids=["all", "gaps"])
def test_both_clis_king_cutoff(tmp_path, host_bin, blocks):
    G = cohort()
    M, N = G.shape
    pre = str(tmp_path / "in")
    iids = [f"s{i}" for i in range(N)]
    gio.write_plink(pre, G, iids, [f"rs{i}" for i in range(M)], ["1"] * M, list(range(1, M + 1)))
    with open(pre + ".fam", "w") as f:
        f.writelines(f"fam{i // 4}\ts{i}\t0\t0\t0\t-9\n" for i in range(N))
    ld = tmp_path / "ld.txt"
    ld.write_text(blocks(M))
    args = ["--eigensnp", "--bed-file", pre + ".bed", "--ld-block-file", str(ld), "--eigensnp-k-global", "3",
            "--eigensnp-max-hwe-p", "1.0", "--gpca-make-king", "--gpca-king-cutoff", "0.0884", "--gpca-save-model"]
    out_py, out_c = str(tmp_path / "py" / "P"), str(tmp_path / "c" / "P")
    assert main(args + ["--out", out_py]) == 0
    r = subprocess.run([host_bin, *args, "--out", out_c], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for ext in (".kin0", ".king.cutoff.in.id", ".king.cutoff.out.id", ".eigensnp.pca.tsv", ".eigenvalues.tsv", ".eigensnp.model.tsv"):
        assert open(out_py + ext, "rb").read() == open(out_c + ext, "rb").read(), ext

    # the table: every pair once, in band order; the planted pairs where they belong
    lines = open(out_py + ".kin0").read().split("\n")
    assert lines[0] == "#FID1\tIID1\tFID2\tIID2\tNSNP\tHETHET\tIBS0\tKINSHIP" and lines[-1] == ""
    rows = [ln.split("\t") for ln in lines[1:-1]]
    assert len(rows) == N * (N - 1) // 2
    idx = {s: i for i, s in enumerate(iids)}
    i1 = np.array([idx[r_[1]] for r_ in rows]); i2 = np.array([idx[r_[3]] for r_ in rows])
    j, k = gio.band_pairs(0, N)
    assert np.array_equal(i1, k) and np.array_equal(i2, j)
    kin = np.array([float(r_[7]) for r_ in rows])
    full = np.zeros((N, N)); full[j, k] = kin; full[k, j] = kin
    for q in range(2):
        b = 200 + 5 * q
        assert full[q * 100 + 5, b] == 0.5                                           # the duplicate
        for par in (b + 1, b + 2):
            for ch in (b + 3, b + 4):
                assert 0.177 <= full[par, ch] <= 0.354
        assert 0.177 <= full[b + 3, b + 4] <= 0.354

    # the out-set: the greedy rule on the table's pairs above the cutoff
    hit = np.flatnonzero(kin > 0.0884)
    inset = gio.king_unrelated(N, list(zip(k[hit], j[hit])))
    want_out = [f"fam{i // 4}\ts{i}" for i in np.flatnonzero(~inset)]
    assert open(out_py + ".king.cutoff.out.id").read().split("\n")[1:-1] == want_out
    assert 4 <= len(want_out) <= 8
    assert open(out_py + ".king.cutoff.in.id").read().count("\n") == 1 + N - len(want_out)

    # every sample is in the score file; the relatives' scores are their projection onto the in-set's PCs
    sc = np.loadtxt(out_py + ".eigensnp.pca.tsv", skiprows=1, usecols=(1, 2, 3))
    assert sc.shape == (N, 3)
    out_q = str(tmp_path / "q" / "Q")
    assert main(["--bed-file", pre + ".bed", "--gpca-project-model", out_py + ".eigensnp.model.tsv", "--out", out_q]) == 0
    pj = np.loadtxt(out_q + ".projected.pca.tsv", skiprows=1, usecols=(1, 2, 3))
    tol = 1e-5 * np.max(np.abs(sc), axis=0)
    assert np.all(np.abs(pj - sc) <= tol + 1e-6)                                   # (+ the two %.6f roundings)
    assert "fit_samples=" + str(int(inset.sum())) in open(out_py + ".eigensnp.model.tsv").readline()
