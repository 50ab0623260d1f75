"""CPU-only: the extent audit of the saddle-point correction's host arithmetic (the asp_* functions of genomic_pca_amd/csrc/plan_math.h).

tests/cpp/assoc_spa_plan_audit.cpp includes the header gpca_assoc_score.cpp sizes the correction's launches and buffers with and walks
k_assoc_spa's index arithmetic by brute force -- every thread of every chunk for 72 sample counts up to 70 000 (the stage, chunk and
slice edges among them), the first and last chunk for sample counts up to 2^30 - 1 -- checking that every 32-sample word and every
sample below the padded count is taken once, that the fetches stay inside a row's pitch, that the LDS buffer, the slices of g~ (within
their byte bound), Z and mu hold every index reached, and that the ranges of the item list cover a band's items once for kept rows up
to 2^31 - 1.  For every one of those sample counts (1024 slots, fewer, and one among them) a forced workgroup count (asp_clamp_slots,
what GPCA_ASP_SLOTS goes through) stays in [1, asp_slots(N)], is the identity on legal values and keeps its slices inside the workspace."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_assoc_spa_extents_fit_and_items_are_covered(tmp_path):
    exe = str(tmp_path / "assoc_spa_plan_audit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "genomic_pca_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "assoc_spa_plan_audit.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("assoc_spa_plan_audit:") and " 0 failures" in last, last
    assert int(last.split()[1]) > 100_000, last      # the grid was walked, not skipped
