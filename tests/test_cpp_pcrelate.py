"""Both command lines on the PC-Relate path: --eigensnp --gpca-make-pcrelate P on a synthetic .bed of two populations with planted
relatives, with and without --gpca-king-cutoff, write byte-identical P.pcrelate.kin and P.pcrelate.inbreed.  The
run hands gpca_pcrelate the first P columns of the scores it writes and, with the cutoff, the KING in-set as the training mask; the
files equal what GpcaEngine.pcrelate gives for that V and train on an engine of the test's own."""
import os
import subprocess

import numpy as np
import pytest

from genomic_pca_amd import _lib
from genomic_pca_amd import io as gio
from genomic_pca_amd.cli import main
from genomic_pca_amd.engine import GpcaEngine, QcConfig

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "genomic_pca_amd", "bin", "genomic_pca")
P = 2


@pytest.fixture(scope="module")
def host_bin():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "genomic_pca_amd", "host"), "-s"])
    return BIN


def cohort(M=3000, n_pop=100, F=0.2, seed=23):
    """two Balding-Nichols populations; per population a duplicate, and a family of two parents and two children (no missing
    calls: the workflow's PCA takes fully called SNPs only, and the missing-call path is held to its bars in test_gpu_pcrelate.py)"""
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


@pytest.fixture(scope="module")
def fileset(tmp_path_factory):
    d = tmp_path_factory.mktemp("pcr")
    G = cohort()
    M, N = G.shape
    pre = str(d / "in")
    gio.write_plink(pre, G, [f"s{i}" for i in range(N)], [f"rs{i}" for i in range(M)], ["1"] * M, list(range(1, M + 1)))
    with open(pre + ".fam", "w") as f:
        f.writelines(f"fam{i // 4}\ts{i}\t0\t0\t0\t-9\n" for i in range(N))
    ld = d / "ld.txt"
    ld.write_text(f"1 1 1200\n1 1501 {M - 200}\n")                  # blocks that leave QC-passing SNPs out of the kept rows
    return pre, str(ld), M, N


@pytest.mark.parametrize("extra", [["--gpca-king-cutoff", "0.0884"],
                                   ["--gpca-pcrelate-maf-bound", "0.03", "--gpca-pcrelate-table-filter", "0.05"]], ids=["inset", "everyone"])
def test_both_clis_pcrelate(tmp_path, host_bin, fileset, monkeypatch, extra):
    pre, ld, M, N = fileset
    args = ["--eigensnp", "--bed-file", pre + ".bed", "--ld-block-file", ld, "--eigensnp-k-global", "3", "--eigensnp-max-hwe-p", "1.0",
            "--gpca-make-pcrelate", str(P), *extra]
    seen = []
    real = GpcaEngine.pcrelate

    def spy(self, pcs, train=None, maf_bound=0.01, rows=None, nsnp=False):
        seen.append((np.array(pcs, np.float64), None if train is None else np.array(train, bool), maf_bound, rows))
        return real(self, pcs, train, maf_bound, rows, nsnp)
    monkeypatch.setattr(GpcaEngine, "pcrelate", spy)
    out_py, out_c = str(tmp_path / "py" / "P"), str(tmp_path / "c" / "P")
    assert main(args + ["--out", out_py]) == 0
    monkeypatch.undo()
    r = subprocess.run([host_bin, *args, "--out", out_c], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for ext in (".pcrelate.kin", ".pcrelate.inbreed", ".eigensnp.pca.tsv"):
        assert open(out_py + ext, "rb").read() == open(out_c + ext, "rb").read(), ext

    # what the run handed gpca_pcrelate: the first P columns of the scores it wrote, and the in-set (or everyone)
    inset_run = extra[0] == "--gpca-king-cutoff"
    assert len(seen) == 1 and seen[0][3] == (0, N)                                  # one band at this size
    V, train, tau, _ = seen[0]
    sc = np.loadtxt(out_py + ".eigensnp.pca.tsv", skiprows=1, usecols=range(1, 1 + P))
    assert V.shape == (N, P) and np.all(np.abs(V - sc) <= 0.5e-6 + 1e-12 * np.abs(V))   # (the file's %.6f rounding)
    assert tau == (0.01 if inset_run else 0.03)
    iids = [f"s{i}" for i in range(N)]
    if inset_run:
        ins = {ln.split("\t")[1] for ln in open(out_py + ".king.cutoff.in.id").read().split("\n")[1:-1]}
        assert train is not None and [s in ins for s in iids] == train.tolist() and 2 <= N - int(train.sum()) <= 8
    else:
        assert train is None

    # the files against GpcaEngine.pcrelate with that V and train, on an engine loaded here: same QC, same kept rows
    fs = gio.read_plink(pre + ".bed")
    with GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=_lib.STORE_INT8) as eng:
        eng.upload_bed2bit(fs.bed_rows, fs.n_samples)
        st = eng.snp_stats(QcConfig(0.98, 0.01, 1.0))
        keep, _ = gio.map_snps_to_ld_blocks(gio.parse_ld_block_file(ld), fs.chromosomes, fs.positions, st["keep"])
        assert 0 < int(keep.sum()) < int(st["keep"].sum())
        eng.set_standardization(st["mu"], st["sigma"], keep)
        kin, cnt = eng.pcrelate(V, train, tau, nsnp=True)
    il = np.tril_indices(N)
    fids = [f"fam{i // 4}" for i in range(N)]
    want = str(tmp_path / "want")
    gio.write_pcrelate(want, fids, iids, [((0, N), kin[il], cnt[il])], None if inset_run else 0.05)
    for ext in (".pcrelate.kin", ".pcrelate.inbreed"):
        assert open(want + ext, "rb").read() == open(out_py + ext, "rb").read(), ext

    # the layout: every strictly lower pair once unless filtered, ID1 the earlier sample; one inbreeding line per sample
    lines = open(out_py + ".pcrelate.kin").read().split("\n")
    assert lines[0] == "#FID1\tIID1\tFID2\tIID2\tNSNP\tKINSHIP" and lines[-1] == ""
    rows = [ln.split("\t") for ln in lines[1:-1]]
    idx = {s: i for i, s in enumerate(iids)}
    assert all(idx[r_[1]] < idx[r_[3]] for r_ in rows)
    if inset_run:
        assert len(rows) == N * (N - 1) // 2
        assert 0 < min(int(r_[4]) for r_ in rows) <= max(int(r_[4]) for r_ in rows) <= int(keep.sum())
    else:
        assert 0 < len(rows) < N * (N - 1) // 2 and all(float(r_[5]) >= 0.05 for r_ in rows)
    inb = open(out_py + ".pcrelate.inbreed").read().split("\n")
    assert inb[0] == "#FID\tIID\tNSNP\tF" and [ln.split("\t")[1] for ln in inb[1:-1]] == iids
