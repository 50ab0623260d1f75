"""CPU-only: the extent audit of the QTL scan's host arithmetic (the qtl_* functions of genomic_pca_amd/csrc/plan_math.h).

tests/cpp/assoc_qtl_plan_audit.cpp includes the header gpca_assoc_qtl.cpp sizes its launches and buffers with and checks, over a sweep
of (rows, N, T, strip width) -- rows up to 2^32, samples up to 2^30 - 1, T from 1 to 2^20 at every tile and strip edge, every legal strip
width and the forced ones, 200 seeded random values per axis -- that the trait panel, yy, the covariate panel, the per-row buffers, the
record buffers and the workspace of the bests hold every index their readers and writers reach, that tiles and strips cover the traits
once and the launches of a band cover its row blocks once, that the grid stays within its bounds, that the workgroup's LDS stays within
the CU's 160 KiB, and that the qtl_* functions agree with asc_npad / asc_lpad / asc_b_capacity where a tile is staged as a 64-column call
of the linear scan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_qtl_extents_fit_and_traits_and_rows_are_covered(tmp_path):
    exe = str(tmp_path / "assoc_qtl_plan_audit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "genomic_pca_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "assoc_qtl_plan_audit.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("assoc_qtl_plan_audit:") and " 0 failures" in last, last
    assert int(last.split()[1]) > 100_000, last      # the grid was walked, not skipped
