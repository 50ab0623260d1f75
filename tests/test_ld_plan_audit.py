"""CPU-only: the extent audit of the windowed-LD host arithmetic (the ld_* functions of genomic_pca_amd/csrc/plan_math.h).

tests/cpp/ld_plan_audit.cpp includes the header gpca_ld.cpp sizes its launches and buffers with and checks, for band sizes up to
2^31 - 1 rows, window widths up to 2^31 - 1 slots and sample counts up to 2^29 - 1 (the tile edges, the limits, and 300 seeded random
values per axis), that the product planes, the per-row sums, r2, counts and the threshold words hold every index their writers reach,
that every in-window pair lies in a tile the kernel multiplies, that the sample stages and their splits cover the samples once, and
that no staged read leaves a row's pitch."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ld_extents_fit_and_band_is_covered(tmp_path):
    exe = str(tmp_path / "ld_plan_audit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "genomic_pca_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ld_plan_audit.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("ld_plan_audit:") and " 0 failures" in last, last
    assert int(last.split()[1]) > 1_000_000, last      # the grid was walked, not skipped
