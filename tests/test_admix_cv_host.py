"""CPU-only: the host side of the admixture cross-validation (include/gpca.h section a22): gpca_admix_cv_fold against a numpy restatement of
the philox rule (_admix_cv.folds_np), io.write_admix_cv against a literal text, and the formats.hpp twin byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib, io as gio
from genomic_pca_amd._lib import GpcaError

from _admix_cv import folds_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("v", [2, 5, 64])
@pytest.mark.parametrize("seed", [0, 1, (1 << 63) - 1])
def test_fold_rule_is_the_philox_restatement(v, seed):
    for N in (1, 257):
        for row0, rows in ((0, 9), (1, 4), (3, 10), (6, 1), (4095, 7), (123457, 5)):
            got = gpca.admix_cv_fold(seed, v, rows, N, row0=row0)
            assert got.dtype == np.uint8 and got.shape == (rows, N)
            assert np.array_equal(got, folds_np(seed, v, rows, N, row0)), (N, row0, rows)
            assert int(got.max()) < v
        # a window is a slice of the whole: the index is global
        assert np.array_equal(gpca.admix_cv_fold(seed, v, 5, N, row0=7), gpca.admix_cv_fold(seed, v, 12, N)[7:])


def test_fold_rule_uses_every_fold_about_equally_and_depends_on_the_seed():
    a, b = gpca.admix_cv_fold(0, 5, 400, 300), gpca.admix_cv_fold(1, 5, 400, 300)
    n = np.bincount(a.ravel(), minlength=5)
    assert n.sum() == 120000 and (np.abs(n - 24000) < 5 * np.sqrt(24000 * 0.8)).all()
    assert 0.15 < (a == b).mean() < 0.25
    assert gpca.admix_cv_fold(0, 2, 0, 7).shape == (0, 7) and gpca.admix_cv_fold(0, 2, 3, 0).shape == (3, 0)
    for bad in (lambda: gpca.admix_cv_fold(0, 1, 4, 4), lambda: gpca.admix_cv_fold(0, 65, 4, 4), lambda: gpca.admix_cv_fold(0, 0, 4, 4),
                lambda: gpca.admix_cv_fold(0, 5, -1, 4), lambda: gpca.admix_cv_fold(0, 5, 4, 4, row0=-1)):
        with pytest.raises(GpcaError) as ei:
            bad()
        assert ei.value.status == _lib.GPCA_ERR_BAD_ARG


ROWS = [
    {"K": 2, "folds": 3, "cv_seed": 7, "fold": 0, "steps": 12, "converged": True, "n_held": 4, "deviance": 5.0},
    {"K": 2, "folds": 3, "cv_seed": 7, "fold": 1, "steps": 30, "converged": False, "n_held": 0, "deviance": 0.0},
    {"K": 2, "folds": 3, "cv_seed": 7, "fold": 2, "steps": 9, "converged": True, "n_held": 3, "deviance": 2.25},
    {"K": 3, "folds": 2, "cv_seed": 18446744073709551615, "fold": 0, "steps": 0, "converged": False, "n_held": 0, "deviance": 0.0},
    {"K": 3, "folds": 2, "cv_seed": 18446744073709551615, "fold": 1, "steps": 0, "converged": False, "n_held": 0, "deviance": float("nan")},
    {"K": 4, "folds": 2, "cv_seed": 0, "fold": 0, "steps": 5, "converged": True, "n_held": 1000000, "deviance": 1136953.4999},
    {"K": 4, "folds": 2, "cv_seed": 0, "fold": 1, "steps": 6, "converged": True, "n_held": 1000000, "deviance": 1136953.5003},
]
TEXT = ("#K\tFOLDS\tCV_SEED\tFOLD\tSTEPS\tCONVERGED\tN_HELD\tDEVIANCE\tCV_ERROR\n"
        "2\t3\t7\t0\t12\t1\t4\t5.000000\t1.250000\n"
        "2\t3\t7\t1\t30\t0\t0\t0.000000\tNA\n"
        "2\t3\t7\t2\t9\t1\t3\t2.250000\t0.750000\n"
        "2\t3\t7\t*\t51\t0\t7\t7.250000\t1.035714\n"
        "3\t2\t18446744073709551615\t0\t0\t0\t0\t0.000000\tNA\n"
        "3\t2\t18446744073709551615\t1\t0\t0\t0\tNA\tNA\n"
        "3\t2\t18446744073709551615\t*\t0\t0\t0\tNA\tNA\n"
        "4\t2\t0\t0\t5\t1\t1000000\t1136953.499900\t1.136953\n"
        "4\t2\t0\t1\t6\t1\t1000000\t1136953.500300\t1.136954\n"
        "4\t2\t0\t*\t11\t1\t2000000\t2273907.000200\t1.136954\n")


def test_write_admix_cv(tmp_path):
    path = gio.write_admix_cv(str(tmp_path / "out"), ROWS)
    assert path.endswith("out.admix.cv") and open(path).read() == TEXT
    assert open(gio.write_admix_cv(str(tmp_path / "none"), [])).read() == TEXT.splitlines(True)[0]


def test_cpp_writer_matches_python(tmp_path):
    """formats.hpp's write_admix_cv against io.write_admix_cv, NaN included"""
    items = ", ".join("{%d, %d, %dull, %d, %d, %s, %d, %s}" % (r["K"], r["folds"], r["cv_seed"], r["fold"], r["steps"], "true" if r["converged"] else "false",
                                                               r["n_held"], "0.0 / 0.0" if r["deviance"] != r["deviance"] else repr(r["deviance"]))
                      for r in ROWS)
    src = tmp_path / "drv.cpp"
    src.write_text('''
#include "formats.hpp"
int main(int argc, char** argv) {
    const std::vector<gpca_host::AdmixCvRow> rows = {''' + items + '''};
    gpca_host::write_admix_cv(std::string(argv[1]), rows);
    gpca_host::write_admix_cv(std::string(argv[1]) + "0", {});
    return 0;
}
''')
    exe = str(tmp_path / "drv")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "genomic_pca_amd", "host"), str(src), "-lz", "-o", exe])
    subprocess.run([exe, str(tmp_path / "c")], check=True, timeout=60)
    assert open(str(tmp_path / "c.admix.cv"), "rb").read() == TEXT.encode()
    assert open(str(tmp_path / "c0.admix.cv"), "rb").read() == TEXT.splitlines(True)[0].encode()
