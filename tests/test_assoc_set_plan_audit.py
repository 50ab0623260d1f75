"""CPU-only: the extent audit of the set call's host arithmetic (kAsg*, asg_* and AsgStrip of genomic_pca_amd/csrc/plan_math.h).

tests/cpp/assoc_set_plan_audit.cpp includes the header gpca_assoc_score.cpp sizes the Gram's launches and buffers with and walks the index
arithmetic of k_assoc_set_gram and k_assoc_set_finish by brute force -- every set size m = 1 .. 128, every strip, every wave's tile and
every accumulator element, whole calls of mixed sets (the GPU test's among them) and the first and last workgroup of calls up to the
grid's limit -- checking that every entry of the packed lower triangle is written once by either kernel and inside phi, that every row
an entry needs is staged, that the listed rows, their sums and dv lie inside their buffers, that every staged read of a row and of the w
column stays inside the row's pitch for sample counts up to 2^30 - 1, and that the sum the GPCA_ERR_OOM check takes equals the sum of the
call's allocations for every combination of outputs."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_assoc_set_extents_fit_and_the_oom_sum_is_the_allocations(tmp_path):
    exe = str(tmp_path / "assoc_set_plan_audit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "genomic_pca_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "assoc_set_plan_audit.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("assoc_set_plan_audit:") and " 0 failures" in last, last
    assert int(last.split()[1]) > 100_000, last      # the grid was walked, not skipped
