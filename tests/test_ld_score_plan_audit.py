"""CPU-only: the extent audit of the LD-score host arithmetic (the ld_score_* functions of genomic_pca_amd/csrc/plan_math.h).

tests/cpp/ld_score_plan_audit.cpp includes the header gpca_ld_score.cpp sizes its launch and buffers with and checks, for bands of up
to 10^7 rows and windows of up to 2^20 slots (the tile edges, the limits and 200 seeded random values per axis), that the grid of
k_ld_score covers the band, that every slot belongs to one thread of one tile and that thread's partner row is the pair's, that the
plane and per-row reads and the two targets of every pair lie inside the buffers the call allocates, and (at compile time) that the
packed (count, sum) words and the 64-bit sums cannot overflow at the largest wmax."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ld_score_extents_fit_and_band_is_covered(tmp_path):
    exe = str(tmp_path / "ld_score_plan_audit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "genomic_pca_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ld_score_plan_audit.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("ld_score_plan_audit:") and " 0 failures" in last, last
    assert int(last.split()[1]) > 1_000_000, last      # the grid was walked, not skipped
