"""Both command lines with --gpca-assoc-spa, on the fileset of tests/test_cpp_assoc_score.py (one case / control trait, one quantitative
trait, a covariate file, --gpca-king-cutoff).  The two programs write byte-identical P.cad.assoc.logistic with the header that ends in
LOG10P SPA, and the file is what GpcaEngine.assoc_logistic_spa gives through io.write_assoc_logistic.  Without the flag the file has
the header and the rows it had before the flag existed: it is the flagged file of --gpca-assoc-spa-z inf (no test corrected: the
normal value everywhere) with the SPA column cut off, byte for byte, and the flagged run at the default cutoff differs from it only
in the LOG10P of the rows marked Y; the linear file of the quantitative trait does not move.  The flag without --gpca-assoc-logistic,
and a cutoff below 0.5, are refused alike by both programs."""
import os
import subprocess

import numpy as np
import pytest

from genomic_pca_amd.cli import main
from genomic_pca_amd.engine import GpcaEngine
from test_cpp_assoc_score import BIN, K_GLOBAL, PCS, fileset, host_bin  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

HEAD = "#CHROM\tPOS\tID\tA1\tOBS_CT\tA1_FREQ\tBETA\tSE\tZ_STAT\tLOG10P"


def test_both_clis_assoc_spa(tmp_path, host_bin, fileset, monkeypatch):
    pre, ld, d, cov, M, N = fileset
    args = ["--eigensnp", "--bed-file", pre + ".bed", "--ld-block-file", ld, "--eigensnp-k-global", str(K_GLOBAL), "--eigensnp-max-hwe-p", "1.0",
            "--gpca-assoc-covar", cov, "--gpca-assoc-pcs", str(PCS), "--gpca-king-cutoff", "0.0884", "--gpca-assoc-pheno",
            os.path.join(d, "t12.pheno"), "--gpca-assoc-logistic"]
    seen = []
    real = GpcaEngine.assoc_logistic_spa

    def spy(self, *a, **kw):
        r = real(self, *a, **kw)
        seen.append((kw.get("spa_z"), r))
        return r
    monkeypatch.setattr(GpcaEngine, "assoc_logistic_spa", spy)
    out_py, out_c, out_inf, out_plain = (str(tmp_path / n / "P") for n in ("py", "c", "inf", "plain"))
    assert main(args + ["--gpca-assoc-spa", "--out", out_py]) == 0
    monkeypatch.undo()
    for extra, out in ((["--gpca-assoc-spa"], out_c), (["--gpca-assoc-spa", "--gpca-assoc-spa-z", "inf"], out_inf), ([], out_plain)):
        r = subprocess.run([host_bin, *args, *extra, "--out", out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
    for ext in (".cad.assoc.logistic", ".height.assoc.linear"):
        assert open(out_py + ext, "rb").read() == open(out_c + ext, "rb").read(), ext
    assert open(out_plain + ".height.assoc.linear", "rb").read() == open(out_c + ".height.assoc.linear", "rb").read()
    spa = open(out_c + ".cad.assoc.logistic").read().split("\n")
    inf = open(out_inf + ".cad.assoc.logistic").read().split("\n")
    plain = open(out_plain + ".cad.assoc.logistic").read().split("\n")
    assert spa[0] == inf[0] == HEAD + "\tSPA" and plain[0] == HEAD and spa[-1] == inf[-1] == plain[-1] == "" and len(spa) == len(inf) == len(plain) > 100
    # no flag = the cutoff inf without its last column, byte for byte
    assert [ln.rsplit("\t", 1)[0] for ln in inf[:-1]] == plain[:-1]
    assert {ln.rsplit("\t", 1)[1] for ln in inf[1:-1]} <= {"N", "NA"}
    # the default cutoff: only the corrected rows' LOG10P moves, and it moves down (the normal value overstates a tail)
    marks = [ln.rsplit("\t", 1)[1] for ln in spa[1:-1]]
    assert set(marks) <= {"N", "Y", "F", "NA"} and marks.count("Y") > 0 and marks.count("N") > marks.count("Y")
    for a, b, m in zip(spa[1:-1], plain[1:-1], marks):
        fa, fb = a.split("\t"), b.split("\t")
        assert fa[:9] == fb[:9]
        if m == "Y":
            assert abs(float(fa[8])) >= 2.0 and float(fa[9]) > 0
        else:
            assert fa[9] == fb[9] and (m == "NA") == (fb[9] == "NA")
    # the file against what the run's own call returned
    assert len(seen) == 1 and seen[0][0] == 2.0
    res = seen[0][1]
    want = ["NA" if v != v else "NYF"[int(s)] for v, s in zip(res["log10p"][:, 0], res["spa_status"][:, 0])]
    assert marks == want
    lp = [float(ln.split("\t")[9]) if ln.split("\t")[9] != "NA" else np.nan for ln in spa[1:-1]]
    assert np.allclose(lp, res["log10p"][:, 0], rtol=1e-5, equal_nan=True)


def test_spa_flag_refusals_are_the_same(host_bin, fileset):
    pre, ld, d, cov, M, N = fileset
    base = ["--eigensnp", "--bed-file", pre + ".bed", "--ld-block-file", ld, "--out", os.path.join(d, "refused"), "--gpca-assoc-pheno",
            os.path.join(d, "t12.pheno")]
    for flags, msg in ((["--gpca-assoc-spa"], "error: --gpca-assoc-spa needs --gpca-assoc-logistic"),
                       (["--gpca-assoc-logistic", "--gpca-assoc-spa", "--gpca-assoc-spa-z", "0.25"],
                        "error: --gpca-assoc-spa-z must be at least 0.5, or inf for no correction")):
        r = subprocess.run([host_bin, *base, *flags], capture_output=True, text=True, timeout=60)
        with pytest.raises(SystemExit) as ei:
            main(base + flags)
        assert r.returncode == 2 and r.stderr == msg + "\n" == str(ei.value) + "\n", (flags, r.stderr)
    assert not os.path.exists(os.path.join(d, "refused.cad.assoc.logistic"))
