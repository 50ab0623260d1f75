"""CPU-only: the extent audit of the admixture step's host arithmetic (the adm_* functions of genomic_pca_amd/csrc/plan_math.h).

tests/cpp/admix_plan_audit.cpp includes the header gpca_admix.cpp sizes its launches and buffers with and walks by brute force every
plan adm_plan returns over a grid of row counts (around the tile of 16 rows and the block of 4 096), sample counts (around the group
of 16, the chunk of 256 and the row pitches), K = 1 .. 16 and CU counts (which the plan does not take: its summation shape is one
function of rows, N and K).  More than 100 000 plans are walked by brute force (the count the program prints as "walked"; the larger
shapes get the closed-form and capacity checks alone): in every walked plan every (row, sample) is read by exactly one thread; every fetch stays inside both row pitches at its
alignment; every LDS index of the three phases stays inside its array; every slab entry is written exactly once and read inside its
capacity; and the GPCA_ERR_OOM sum equals the allocations."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_admix_extents_fit_and_every_call_is_read_once(tmp_path):
    exe = str(tmp_path / "admix_plan_audit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "genomic_pca_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "admix_plan_audit.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("admix_plan_audit:") and " 0 failures" in last, last
    assert int(last.split()[1]) > 100_000 and int(last.split()[5]) > 100_000, last       # checks made; plans walked by brute force
