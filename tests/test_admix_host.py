"""CPU-only: the host rules around the admixture fit (genomic_pca_amd/io.py: admix_order, admix_supervised, write_admix; gpca.h section
a21) against hand-written expectations."""
import numpy as np
import pytest

from genomic_pca_amd import io as gio


def test_admix_order():
    Q = np.array([[0.1, 0.6, 0.3], [0.2, 0.5, 0.3], [0.3, 0.3, 0.4]], np.float32)       # sums 0.6, 1.4, 1.0
    assert gio.admix_order(Q).tolist() == [1, 2, 0] and gio.admix_order(Q).dtype == np.int64
    assert gio.admix_order(Q, np.zeros(3, np.uint8)).tolist() == [1, 2, 0]
    assert gio.admix_order(Q, np.array([0, 2, 2], np.uint8)).tolist() == [1, 2, 0]       # mode 2 counts like mode 0
    assert gio.admix_order(Q, np.array([0, 1, 0], np.uint8)).tolist() == [0, 1, 2]       # supervised: the identity
    tie = np.array([[0.25, 0.5, 0.25], [0.25, 0.5, 0.25]], np.float32)
    assert gio.admix_order(tie).tolist() == [1, 0, 2]                                    # ties to the lower index
    assert gio.admix_order(np.full((4, 5), 0.2, np.float32)).tolist() == [0, 1, 2, 3, 4]
    assert gio.admix_order(np.ones((3, 1), np.float32)).tolist() == [0]
    with pytest.raises(ValueError):
        gio.admix_order(Q, np.zeros(2, np.uint8))
    with pytest.raises(ValueError):
        gio.admix_order(np.zeros(3))


def test_admix_supervised():
    eps = np.float32(1e-5)
    Q, mode = gio.admix_supervised([2, -1, 0, -9], 3)
    assert Q.dtype == np.float32 and mode.dtype == np.uint8 and mode.tolist() == [1, 0, 1, 0]
    s = np.float32(np.float32(eps + eps) + np.float32(1))
    assert np.array_equal(Q[0], np.array([eps, eps, 1], np.float32) / s)
    s = np.float32(np.float32(np.float32(1) + eps) + eps)
    assert np.array_equal(Q[2], np.array([1, eps, eps], np.float32) / s)
    third = np.float32(1.0) / np.float32(3)
    assert np.array_equal(Q[1], np.full(3, third, np.float32)) and np.array_equal(Q[3], Q[1])
    assert Q[0].min() > 0 and abs(float(Q[0].astype(np.float64).sum()) - 1) < 3 * 2.0 ** -24
    given = np.arange(12, dtype=np.float32).reshape(4, 3)
    Q2, mode2 = gio.admix_supervised([2, -1, 0, -9], 3, given)
    assert np.array_equal(Q2[[1, 3]], given[[1, 3]]) and np.array_equal(Q2[[0, 2]], Q[[0, 2]]) and np.array_equal(mode2, mode)
    assert given[0, 0] == 0                                                              # the caller's array is not written
    Q1, m1 = gio.admix_supervised([0, 0], 1)
    assert np.array_equal(Q1, np.ones((2, 1), np.float32)) and m1.tolist() == [1, 1]
    for bad in (lambda: gio.admix_supervised([3], 3), lambda: gio.admix_supervised([0], 0), lambda: gio.admix_supervised([0], 2, np.zeros((2, 2)))):
        with pytest.raises(ValueError):
            bad()


def test_write_admix(tmp_path):
    Q = np.array([[0.25, 0.75], [0.9999996, 0.0000004], [0.00001, 0.99999]], np.float32)
    F = np.array([[0.5, 0.125], [1e-5, 1 - 1e-5]], np.float32)
    info = {"seed": 42, "steps": 17, "cycles": 6, "converged": True, "loglik": -1234.56789}
    paths = gio.write_admix(str(tmp_path / "out"), 2, ["f1", "f2", "f3"], ["i1", "i2", "i3"], ["rs1", "rs2"], Q, F, info)
    assert [p.rsplit("/", 1)[1] for p in paths] == ["out.2.Q", "out.2.Q.id", "out.2.P", "out.2.P.id", "out.2.admix.log"]
    text = [open(p).read() for p in paths]
    assert text[0] == "0.250000 0.750000\n1.000000 0.000000\n0.000010 0.999990\n"
    assert text[1] == "#FID\tIID\nf1\ti1\nf2\ti2\nf3\ti3\n"
    assert text[2] == "0.500000 0.125000\n0.000010 0.999990\n"
    assert text[3] == "rs1\nrs2\n"
    assert text[4] == "#K\tSEED\tSTEPS\tCYCLES\tCONVERGED\tLOGLIK\n2\t42\t17\t6\t1\t-1234.5679\n"
    info["converged"] = False
    gio.write_admix(str(tmp_path / "out"), 2, ["f1", "f2", "f3"], ["i1", "i2", "i3"], ["rs1", "rs2"], Q, F, info)
    assert open(paths[4]).read().endswith("\t0\t-1234.5679\n")
    for bad in (lambda: gio.write_admix(str(tmp_path / "x"), 3, ["f1", "f2", "f3"], ["i1", "i2", "i3"], ["rs1", "rs2"], Q, F, info),
                lambda: gio.write_admix(str(tmp_path / "x"), 2, ["f1"], ["i1", "i2", "i3"], ["rs1", "rs2"], Q, F, info),
                lambda: gio.write_admix(str(tmp_path / "x"), 2, ["f1", "f2", "f3"], ["i1", "i2", "i3"], ["rs1"], Q, F, info)):
        with pytest.raises(ValueError):
            bad()
