"""CPU-only: the extent audit of the cis-QTL call's host arithmetic (the qtl_cis_* and qtl_perm_* functions of
genomic_pca_amd/csrc/plan_math.h).

tests/cpp/assoc_qtl_cis_plan_audit.cpp includes the header gpca_assoc_qtl_cis.cpp sizes its launches and buffers with and checks, over a
sweep of (N, n, P, Pc, G) and of windows inside a union of windows -- P from 0 to 65 535 at every tile edge, samples at and around the
LDS limit of the panel kernel, windows from one row to 2^31, seeded random values per axis -- that the panel, the table, Q, the residuals,
the bests of a launch, the running best and the [G][P] result hold every index their readers and writers reach, that the workgroups of
the panel kernel cover the P + 1 columns once, that the launches of a window cover its row blocks once from lo and read only the union's
per-row buffers, and that the static LDS of both kernels stays within 64 KiB."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_qtl_cis_extents_fit_and_columns_and_windows_are_covered(tmp_path):
    exe = str(tmp_path / "assoc_qtl_cis_plan_audit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "genomic_pca_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "assoc_qtl_cis_plan_audit.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("assoc_qtl_cis_plan_audit:") and " 0 failures" in last, last
    assert int(last.split()[1]) > 100_000, last      # the grid was walked, not skipped
