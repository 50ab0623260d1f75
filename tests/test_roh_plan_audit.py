"""CPU-only: the extent audit of the runs-of-homozygosity host arithmetic (the roh_* functions of genomic_pca_amd/csrc/plan_math.h).

tests/cpp/roh_plan_audit.cpp includes the header gpca_roh.cpp sizes its launches and buffers with and walks by brute force every plan
roh_plan returns over a grid of row counts (around the default window of 50, the widest of 64 and the 256-row split), sample counts
(around the thread's 16 samples, the wave's 1 024 and the row pitches), windows (1, 2, 5, 50, 63, 64), CU counts, forced split counts
(1, 2, 3, 7, rows, and values above the rows) and domain layouts (one domain, every row a domain, lengths W - 1 .. 2 W, random): every
row of the band is decided by exactly one split with the coverage a20 states; every halo row and every second fetch stays inside the
band and its domain, and every fetch inside both row pitches with the alignment its load needs; every plane and count entry is written
once and read inside its capacity; the GPCA_ERR_OOM sum equals the allocations; and no counter can wrap."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_roh_extents_fit_and_every_row_is_decided_once(tmp_path):
    exe = str(tmp_path / "roh_plan_audit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "genomic_pca_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "roh_plan_audit.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("roh_plan_audit:") and " 0 failures" in last, last
    assert int(last.split()[1]) > 100_000, last      # the grid was walked, not skipped
