"""CPU-only: the extent audit of the per-sample genotype counts' host arithmetic (the sc_* functions of genomic_pca_amd/csrc/plan_math.h).

tests/cpp/sample_counts_plan_audit.cpp includes the header gpca_sample_counts.cpp sizes its launch and buffers with and walks by brute
force every plan sc_plan returns over a grid of row counts (around the fetch group of 8, the byte counters' flush at 248 and 255),
sample counts (around the thread's 16 samples, the wave's 1 024 and the row pitches), CU counts and forced split counts (1, 2, 3, 7,
rows, and values above the rows): every (row, sample) of the band is read by exactly one thread; every fetch stays inside both row
pitches with the alignment its vector load needs; every slab entry is written exactly once and read inside its capacity; the
GPCA_ERR_OOM sum equals the allocations; and no counter can wrap."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sample_counts_extents_fit_and_every_call_is_read_once(tmp_path):
    exe = str(tmp_path / "sample_counts_plan_audit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "genomic_pca_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "sample_counts_plan_audit.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("sample_counts_plan_audit:") and " 0 failures" in last, last
    assert int(last.split()[1]) > 100_000, last      # the grid was walked, not skipped
