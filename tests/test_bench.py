"""bench.py's own contract: a plain run times the headline path only and `--full` adds the rest of the line; `--dump-outputs DIR`
writes what the headline path returned after its last timed step, the same bits for the same arguments in every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--snps", "60000", "--samples", "2048", "--steps", "3", "--warmup", "1"]
FULL_ONLY = ("f32_mfma_path", "packed_2bit_residency", "packed_2bit_four_planes", "parity")


def _bench(args, timeout=600):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_dump_outputs_caps_large_arrays_with_a_fixed_sample(tmp_path):
    """No GPU: an engine stand-in with 1M x 20 loadings (80 MB) and 500k x 20 scores (80 MB): both are cut to a seeded sample of
    their rows, the same rows in every call, and the files stay under 64 MB in all."""
    sys.path.insert(0, ROOT)
    import bench

    class Eng:
        def eigenvalues(self):
            return np.arange(20, 0, -1, dtype=np.float64)

        def singular_values(self):
            return np.arange(30, 0, -1, dtype=np.float64)

        def scores(self, f64=False):
            return np.arange(500_000 * 20, dtype=np.float64).reshape(500_000, 20)

        def loadings(self):
            return np.arange(1_000_000 * 20, dtype=np.float32).reshape(1_000_000, 20)

    bench.dump_outputs(Eng(), str(tmp_path / "a"))
    bench.dump_outputs(Eng(), str(tmp_path / "b"))
    total = 0
    for name, dtype in (("eigenvalues", np.float64), ("singular_values", np.float64), ("scores", np.float64), ("loadings", np.float32)):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == dtype and np.array_equal(a, b)
        total += os.path.getsize(tmp_path / "a" / f"{name}.npy")
    assert total <= 64 << 20
    sc, ld = np.load(tmp_path / "a" / "scores.npy"), np.load(tmp_path / "a" / "loadings.npy")
    assert 0 < sc.shape[0] < 500_000 and 0 < ld.shape[0] < 1_000_000 and sc.shape[1] == ld.shape[1] == 20
    rows = ld[:, 0] / 20                          # the sampled rows, in increasing order, each row whole
    assert np.all(np.diff(rows) > 0) and np.array_equal(ld, np.arange(20, dtype=np.float32) + (rows * 20)[:, None])


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_run_times_the_headline_only_and_full_adds_the_rest():
    d = _bench(SMALL)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["higher_is_better"] is True
    assert d["value"] == pytest.approx(60000 * 2048 / (d["ms_per_step"] * 1e-3)) and d["roofline"]["launches"] > 0
    assert d["cpu_baseline"] is None and not [k for k in FULL_ONLY if k in d]
    f = _bench(SMALL + ["--full", "--no-cpu-baseline"])      # (--no-cpu-baseline drops parity with it)
    assert [k for k in FULL_ONLY if k in f] == [k for k in FULL_ONLY if k != "parity"] and "extra_path_errors" not in f
    assert f["cpu_baseline"] is None and f["f32_mfma_path"]["max_rel_d_eigenvalue_vs_default_path"] < 1e-4
    assert f["top_eigenvalues"] == d["top_eigenvalues"] and f["dtype"] == d["dtype"] and f["metric"] == d["metric"]


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_dumped_outputs_are_the_last_steps_and_repeat_bit_for_bit(tmp_path):
    runs = []
    for name in ("a", "b"):
        d = _bench(SMALL + ["--dump-outputs", str(tmp_path / name)])
        runs.append({n: np.load(tmp_path / name / f"{n}.npy") for n in ("eigenvalues", "singular_values", "scores", "loadings")})
        assert np.array_equal(runs[-1]["eigenvalues"][:3], d["top_eigenvalues"])
    a, b = runs
    assert a["eigenvalues"].shape == (20,) and a["singular_values"].shape == (30,)
    assert a["scores"].shape == (2048, 20) and a["scores"].dtype == np.float64
    assert 0 < a["loadings"].shape[0] <= 60000 and a["loadings"].shape[1] == 20 and a["loadings"].dtype == np.float32   # (PCA SNPs)
    for n in a:
        assert np.array_equal(a[n], b[n]), n
