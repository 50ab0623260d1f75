"""CPU-only: io.ld_score_sum and the writers of the LD-score files (io.write_ldscore, io.write_ldsc_summary) on small hand-made inputs:
the sums at their offsets, exact file bytes and the NA rules."""
import numpy as np
import pytest

from genomic_pca_amd import io as gio


def test_ld_score_sum_adds_bands_at_their_row0():
    K = 9
    b0 = ((0, 3), np.array([10, 20, 30, 5, 7], np.int64), np.array([1, 2, 3, 1, 1], np.int32))          # span 5: reaches rows 3, 4
    b1 = ((3, 7), np.array([100, 200, 300, 400, -50, 9], np.int64), np.array([2, 2, 2, 2, 1, 1], np.int32))
    b2 = ((7, 9), np.array([1, 2], np.int64))                                                          # no partners given
    acc, part = gio.ld_score_sum(K, [b0, b1, b2])
    assert acc.dtype == np.int64 and part.dtype == np.int64
    assert acc.tolist() == [10, 20, 30, 105, 207, 300, 400, -49, 11]
    assert part.tolist() == [1, 2, 3, 3, 3, 2, 2, 1, 1]
    acc2, part2 = gio.ld_score_sum(K, [b2, b1, b0])                                                    # any order
    assert np.array_equal(acc, acc2) and np.array_equal(part, part2)
    big = ((0, 1), np.array([2 ** 62 - 1], np.int64))                                                  # int64 all the way (no float in between)
    assert gio.ld_score_sum(1, [big, ((0, 1), np.array([-(2 ** 62) + 2], np.int64))])[0].tolist() == [1]
    acc0, part0 = gio.ld_score_sum(4, [])
    assert acc0.tolist() == [0, 0, 0, 0] and part0.tolist() == [0, 0, 0, 0]
    assert gio.ld_score_sum(3, [((1, 1), np.zeros(0, np.int64))])[0].tolist() == [0, 0, 0]              # an empty band
    with pytest.raises(ValueError):
        gio.ld_score_sum(4, [((2, 4), np.zeros(3, np.int64))])                                          # past K
    with pytest.raises(ValueError):
        gio.ld_score_sum(4, [((0, 2), np.zeros(2))])                                                    # not integers
    with pytest.raises(ValueError):
        gio.ld_score_sum(4, [((0, 2), np.zeros(2, np.int64), np.zeros(3, np.int32))])


def test_write_ldscore_bytes(tmp_path):
    prefix = str(tmp_path / "sub" / "run")
    l2 = [1.0, 12.3456789, 1.0 + 2.0 ** -40, 123456789.0, float("nan")]
    maf = [0.5, 0.05, 0.0500001, 0.01, 0.2]
    paths = gio.write_ldscore(prefix, ["1", "1", "2", "X", "X"], ["rs1", "rs2", "rs3", "rs4", "rs5"], [100, 2000, 5, 7, 9], l2, maf)
    assert paths == [prefix + ".l2.ldscore", prefix + ".l2.M", prefix + ".l2.M_5_50"]
    assert open(paths[0], "rb").read() == (b"CHR\tSNP\tBP\tL2\n1\trs1\t100\t1\n1\trs2\t2000\t12.3457\n2\trs3\t5\t1\nX\trs4\t7\t1.23457e+08\n"
                                           b"X\trs5\t9\tNA\n")
    assert open(paths[1], "rb").read() == b"5\n"
    assert open(paths[2], "rb").read() == b"3\n"                             # MAF > 0.05, strictly
    with pytest.raises(ValueError):
        gio.write_ldscore(prefix, ["1"], ["a", "b"], [1, 2], [1.0, 1.0], [0.1, 0.1])
    empty = gio.write_ldscore(str(tmp_path / "none"), [], [], [], [], [])
    assert open(empty[0], "rb").read() == b"CHR\tSNP\tBP\tL2\n" and open(empty[1], "rb").read() == b"0\n" and open(empty[2], "rb").read() == b"0\n"


def test_write_ldsc_summary_bytes(tmp_path):
    prefix = str(tmp_path / "run")
    nan = float("nan")
    fit = {"m_used": 1234, "mean_chi2": 1.5, "lambda_gc": 1.23456789, "intercept": 1.02, "intercept_se": 0.0123456789, "h2": 0.4, "h2_se": 1e-5,
           "ratio": 0.04, "ratio_se": 0.0246913578, "n_blocks": 200}
    low = dict(fit, mean_chi2=0.98, ratio=nan, ratio_se=nan, h2=-0.01)
    path = gio.write_ldsc_summary(prefix, [("height", "LINEAR", 5000, fit), ("case", "LOGISTIC", 4990, low), ("thin", "LINEAR", 12, None)])
    assert path == prefix + ".ldsc.summary"
    assert open(path, "rb").read() == (
        b"#TRAIT\tTEST\tN\tM_USED\tMEAN_CHI2\tLAMBDA_GC\tINTERCEPT\tINTERCEPT_SE\tH2\tH2_SE\tRATIO\tRATIO_SE\n"
        b"height\tLINEAR\t5000\t1234\t1.5\t1.23457\t1.02\t0.0123457\t0.4\t1e-05\t0.04\t0.0246914\n"
        b"case\tLOGISTIC\t4990\t1234\t0.98\t1.23457\t1.02\t0.0123457\t-0.01\t1e-05\tNA\tNA\n"
        b"thin\tLINEAR\t12\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n")
    with pytest.raises(ValueError):
        gio.write_ldsc_summary(prefix, [("t", "FIRTH", 1, fit)])
    assert open(gio.write_ldsc_summary(prefix, []), "rb").read() == b"#TRAIT\tTEST\tN\tM_USED\tMEAN_CHI2\tLAMBDA_GC\tINTERCEPT\tINTERCEPT_SE\tH2\tH2_SE\tRATIO\tRATIO_SE\n"
