"""CPU-only: the extent audit of the engine's host arithmetic (genomic_pca_amd/csrc/plan_math.h).

tests/cpp/plan_audit.cpp includes the header the engine itself sizes its launches and workspaces with, and checks, for every sketch
width L in {32, 64, 128}, row counts up to 1e8 and sample counts up to 4 194 304 (the tile and padding edges, the points where the
Gram's part count jumps, and 300 seeded random values per axis), that every writer's extent fits the buffer it writes, that every
GEMM plan covers every row and sample exactly once, and that every single-workgroup fold stays inside its documented limit.

With the buffer sizes the engine had before plan_math.h existed the audit reports, among others,
    FAIL d_scratch64 <- Gram of B (gram_num_parts(M)): L=128 M=2097153: parts=1025 S=17 writes 278528 doubles into a buffer of 262144
(a sketch of 65..128 columns on more than 2 097 152 rows wrote past the 2 MiB scratch of the two-stage sum).  To see it again: in a
copy of plan_math.h let sum_scratch_capacity return 64 * 4096 and part64_capacity use gram_num_parts(M) in place of gram_max_parts, and
build the audit with -I pointing at the copy."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "plan_audit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "genomic_pca_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "plan_audit.cpp"), "-o", exe])
    return exe


def test_every_extent_fits_and_every_plan_covers(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=600)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("plan_audit:") and " 0 failures" in last, last
    assert int(last.split()[1]) > 1_000_000, last      # the grid was walked, not skipped
