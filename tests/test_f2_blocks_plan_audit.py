"""CPU-only: the extent audit of the f2 jackknife blocks' host arithmetic (the fb_* functions of genomic_pca_amd/csrc/plan_math.h).

tests/cpp/f2_blocks_plan_audit.cpp includes the header gpca_f2_blocks.cpp sizes its launch and buffers with and walks by brute force:
the pair map is a bijection onto 0 .. pairs - 1 for every P from 2 to 64, its inverse is the one the kernel uses, and every pair has
exactly one (thread, register slot) owner under the launcher's slot counts; for row counts around the LDS tile (32) and the
workgroup's run (256) up to the 2^21 rows a call accepts, every read of the counts workspace and of the block ids stays inside its
buffer, every LDS word a pair reads was written exactly once in its tile and stays inside the tile's planes, and every output index
stays inside [B][pairs]; the GPCA_ERR_OOM sum equals the allocations; and a call's i64 sums stay below 2^63 and its counts below 2^31."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_f2_blocks_extents_fit_and_the_pair_map_is_a_bijection(tmp_path):
    exe = str(tmp_path / "f2_blocks_plan_audit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "genomic_pca_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "f2_blocks_plan_audit.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("f2_blocks_plan_audit:") and " 0 failures" in last, last
    assert int(last.split()[1]) > 100_000, last      # the grid was walked, not skipped
