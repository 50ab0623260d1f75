"""CPU-only: the extent audit of the per-group genotype counts' host arithmetic (the gc_* functions of genomic_pca_amd/csrc/plan_math.h).

tests/cpp/group_counts_plan_audit.cpp includes the header gpca_group_counts.cpp sizes its launch and buffers with and walks by brute
force, for sample counts up to 2^30 - 1 (every stage up to 4 096 samples, the first and last three beyond) and every P from 1 to 64:
every thread's staged read of a row stays inside both row pitches and every staged read of the one-hot matrix inside its column and its
buffer, with the alignment the vector loads need; every LDS read and write stays inside its stage buffer; every counts entry of a band
(row counts and offsets around the wave's 32 rows and the workgroup's 128) is written exactly once, inside the buffer; the
GPCA_ERR_OOM sum equals the allocations; and no i32 accumulator can pass 2^31 - 1."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_counts_extents_fit_and_every_count_is_written_once(tmp_path):
    exe = str(tmp_path / "group_counts_plan_audit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "genomic_pca_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "group_counts_plan_audit.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("group_counts_plan_audit:") and " 0 failures" in last, last
    assert int(last.split()[1]) > 100_000, last      # the grid was walked, not skipped
