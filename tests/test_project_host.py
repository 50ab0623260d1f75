"""Host side of the projection path (no GPU): the model file, the alignment of a model to a target .bim, the .bim alleles of
read_plink, and the argument errors of the new CLI flags."""
import os

import numpy as np
import pytest

from genomic_pca_amd import cli
from genomic_pca_amd import io as gio


def _model(ids, a1, a2, k=3, seed=0):
    rng = np.random.default_rng(seed)
    S = len(ids)
    return gio.ProjectionModel(list(ids), ["1"] * S, list(range(100, 100 + S)), list(a1), list(a2),
                               rng.uniform(0.05, 1.95, S).astype(np.float32), rng.uniform(0.1, 1.0, S).astype(np.float32),
                               (rng.standard_normal((S, k)) * 1e-3).astype(np.float32), np.array([3.25, 1.0 / 3.0, 1e-7][:k]), 1234)


def test_model_roundtrip_f32_exact(tmp_path):
    ids = [f"rs{i}" for i in range(50)]
    m = _model(ids, ["A"] * 50, ["G"] * 50)
    m.mean[0] = np.float32(np.nextafter(np.float32(1.0), np.float32(2.0)))
    m.loadings[1, 2] = np.float32(-1.1754944e-38)
    path = gio.write_model(str(tmp_path / "P"), m)
    assert path.endswith("P.eigensnp.model.tsv")
    r = gio.read_model(path)
    assert r.variant_ids == m.variant_ids and r.allele1 == m.allele1 and r.allele2 == m.allele2 and r.positions == m.positions
    assert r.mean.dtype == np.float32 and np.array_equal(r.mean, m.mean) and np.array_equal(r.sd, m.sd)
    assert np.array_equal(r.loadings, m.loadings)
    assert np.array_equal(r.eigenvalues, m.eigenvalues) and r.n_samples == 1234 and r.k == 3
    lines = open(path).read().splitlines()
    assert lines[0] == "#gpca-model v1\tk=3\tfit_samples=1234"
    assert lines[1].startswith("#eigenvalues\t3.25\t")
    assert lines[2] == "VariantID\tChrom\tPos\tA1\tA2\tMean\tSD\tPC1_loading\tPC2_loading\tPC3_loading"


def test_read_model_rejects_other_files(tmp_path):
    p = tmp_path / "x.tsv"
    p.write_text("VariantID\tChrom\tPos\n")
    with pytest.raises(ValueError):
        gio.read_model(str(p))


def test_align_flip_absent_mismatch_duplicates_dot():
    m = _model(["a", "b", "c", "d", ".", "e"], ["A", "C", "A", "T", "A", "G"], ["G", "T", "G", "C", "G", "A"])
    # target: b swapped, a as is, c with another allele pair, d absent, '.' never matches, e twice (the first wins, swapped)
    tid = ["x", "b", "a", "c", ".", "e", "e"]
    t1 = ["A", "T", "A", "A", "A", "A", "G"]
    t2 = ["G", "C", "G", "T", "G", "G", "A"]
    al = gio.align_model(m, tid, t1, t2)
    assert (al.matched, al.flipped, al.allele_mismatch, al.absent) == (3, 2, 1, 2)
    assert np.array_equal(al.loadings[2], m.loadings[0]) and al.mean[2] == m.mean[0]          # a: as is
    assert np.array_equal(al.loadings[1], -m.loadings[1]) and al.mean[1] == np.float32(2) - m.mean[1]   # b: flipped
    assert np.array_equal(al.loadings[5], -m.loadings[5])                                       # e: first occurrence, flipped
    for i in (0, 3, 4, 6):                                                                       # x, c (mismatch), '.', second e
        assert not np.any(al.loadings[i])
    assert al.sd[1] == m.sd[1]


def test_read_plink_alleles(tmp_path):
    G = np.array([[0, 1, 2], [2, -127, 0]], np.int8)
    pre = str(tmp_path / "t")
    gio.write_plink(pre, G, ["s1", "s2", "s3"], ["v1", "v2"], ["1", "2"], [10, 20], alleles=[("A", "C"), ("TT", "G")])
    fs = gio.read_plink(pre + ".bed")
    assert fs.allele1 == ["A", "TT"] and fs.allele2 == ["C", "G"]
    assert fs.variant_ids == ["v1", "v2"] and list(fs.positions) == [10, 20]
    gio.write_plink(pre, G, ["s1", "s2", "s3"], ["v1", "v2"], ["1", "2"], [10, 20])          # default alleles unchanged
    assert open(pre + ".bim").read().splitlines()[0] == "1\tv1\t0\t10\tA\tG"


def test_write_projected_format(tmp_path):
    p = gio.write_projected(str(tmp_path / "Q"), ["a", "b"], np.array([[1.0, -0.5], [0.0, 2.25]]), [7, 0])
    assert open(p).read() == "SampleID\tPC1\tPC2\tSNPsUsed\na\t1.000000\t-0.500000\t7\nb\t0.000000\t2.250000\t0\n"


def test_cli_argument_errors(tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.main(["--out", str(tmp_path / "Q"), "--gpca-project-model", "m.tsv"])
    assert "--bed-file" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(["--out", str(tmp_path / "Q"), "--gpca-save-model", "-d", str(tmp_path), "-k", "2"])
    assert "--eigensnp" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(["--out", str(tmp_path / "Q"), "--gpca-project-model", "m.tsv", "--bed-file", "t.bed", "--eigensnp"])
    assert "--eigensnp" in str(e.value)


def test_cli_no_matching_snp(tmp_path):
    m = _model(["a", "b"], ["A", "A"], ["G", "G"])
    mp = gio.write_model(str(tmp_path / "P"), m)
    pre = str(tmp_path / "t")
    gio.write_plink(pre, np.zeros((2, 4), np.int8), ["s1", "s2", "s3", "s4"], ["z1", "z2"], ["1", "1"], [1, 2])
    with pytest.raises(SystemExit) as e:
        cli.main(["--out", str(tmp_path / "Q"), "--gpca-project-model", mp, "--bed-file", pre + ".bed"])
    assert "no SNP" in str(e.value)
    assert not os.path.exists(str(tmp_path / "Q.projected.pca.tsv"))
