"""CPU-only: the extent audit of the Firth correction's host arithmetic (afi_out_capacity, the asp_* functions as the new call uses them
and asr_call_bytes of genomic_pca_amd/csrc/plan_math.h).

tests/cpp/assoc_firth_plan_audit.cpp includes the header gpca_assoc_score.cpp sizes the correction's launches and buffers with and walks
the index arithmetic of k_assoc_firth_flag and k_assoc_firth by brute force -- every thread of the flag kernel for bands up to 100 000
rows (the GPU test's 70 000 x 16 across the 2^20-item list range among them), the first and last workgroup of every range up to
2^31 - 1 rows -- checking that every item is flagged once, that its five results, its z, its row's sums and its list entry lie inside
their buffers, that the slices of g~, Z and mu hold every sample a pass reaches for sample counts up to 2^30 - 1, and that the sum
the GPCA_ERR_OOM check takes equals the sum of the call's allocations for every combination of outputs, correction and cutoff."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_assoc_firth_extents_fit_and_the_oom_sum_is_the_allocations(tmp_path):
    exe = str(tmp_path / "assoc_firth_plan_audit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "genomic_pca_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "assoc_firth_plan_audit.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("assoc_firth_plan_audit:") and " 0 failures" in last, last
    assert int(last.split()[1]) > 100_000, last      # the grid was walked, not skipped
