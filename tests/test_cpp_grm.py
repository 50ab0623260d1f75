"""Both command lines on the GRM path: --eigensnp --gpca-make-grm on a synthetic .bed with 3 % missing calls writes byte-identical
P.grm.bin / P.grm.N.bin / P.grm.id through each; the values are the numpy GRM of the kept SNPs up to f32 rounding.  (The workflow's
PCA refuses a missing call in a PCA SNP, so the missing calls sit in rows that the call-rate filter or the LD blocks leave out.)"""
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


@pytest.mark.parametrize("scaling", ["standardized", "centred"])
def test_both_clis_write_the_same_grm(tmp_path, host_bin, scaling):
    M, N = 3000, 257
    rng = np.random.default_rng(23)
    p = rng.uniform(0.05, 0.5, size=(M, 1))
    G = (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)
    bad = rng.random(M) < 0.1                                      # 10 % of the rows: 25 % missing (fail the 0.98 call rate)
    bad[2500:] = True                                              # rows outside every block: 5 % missing
    rate = np.where(np.arange(M) < 2500, 0.25, 0.05)[:, None] * bad[:, None]
    G[rng.random((M, N)) < rate] = -127
    assert 0.02 < np.mean(G == -127) < 0.04
    pre = str(tmp_path / "in")
    iids = [f"s{i}" for i in range(N)]
    gio.write_plink(pre, G, iids, [f"rs{i}" for i in range(M)], ["1"] * M, list(range(1, M + 1)))
    with open(pre + ".fam", "w") as f:
        f.writelines(f"fam{i // 3}\ts{i}\t0\t0\t0\t-9\n" for i in range(N))
    ld = tmp_path / "ld.txt"
    ld.write_text("1 1 1500\n1 1501 2500\n")                      # rows past 2 500 are outside every block: not kept
    args = ["--eigensnp", "--bed-file", pre + ".bed", "--ld-block-file", str(ld), "--eigensnp-k-global", "3",
            "--eigensnp-max-hwe-p", "1.0", "--gpca-make-grm", "--gpca-grm-scaling", scaling]
    out_py, out_c = str(tmp_path / "py" / "P"), str(tmp_path / "c" / "P")
    assert main(args + ["--out", out_py]) == 0
    r = subprocess.run([host_bin, *args, "--out", out_c], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for ext in (".grm.bin", ".grm.N.bin", ".grm.id"):
        assert open(out_py + ext, "rb").read() == open(out_c + ext, "rb").read(), ext
    assert open(out_py + ".grm.id").read() == "".join(f"fam{i // 3}\ts{i}\n" for i in range(N))

    # numpy: the rows that pass QC (MAF 0.01, call rate 0.98) and fall in a block
    X = G[:2500]
    obs = X != -127
    cnt = obs.sum(axis=1)
    mu = np.where(obs, X, 0).sum(axis=1) / cnt
    sd = np.sqrt(np.where(obs, (X - mu[:, None]) ** 2, 0).sum(axis=1) / (cnt - 1))
    maf = np.minimum(mu / 2, 1 - mu / 2)
    keep = (cnt / N >= 0.98) & (maf >= 0.01) & (sd > 0)
    assert 2000 < keep.sum() < 2400
    X, obs, mu, sd = X[keep], obs[keep], mu[keep], sd[keep]
    Z = X - mu[:, None]
    if scaling == "standardized":
        Z = Z / sd[:, None]
    Z = np.where(obs, Z, 0.0)
    ref = (Z.T @ Z) / Z.shape[0]
    o = obs.astype(np.float64)
    il = np.tril_indices(N)
    g = np.fromfile(out_py + ".grm.bin", dtype="<f4")
    n = np.fromfile(out_py + ".grm.N.bin", dtype="<f4")
    assert g.size == N * (N + 1) // 2
    assert np.max(np.abs(g - ref[il])) <= 1e-5 * np.max(np.diag(ref))
    assert np.array_equal(n, (o.T @ o)[il].astype(np.float32))
