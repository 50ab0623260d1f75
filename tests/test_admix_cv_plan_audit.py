"""CPU-only: the extent audit of the hold-out step's host arithmetic (the adm_cv_* functions of genomic_pca_amd/csrc/plan_math.h;
include/gpca.h section a22).

tests/cpp/admix_cv_plan_audit.cpp includes the header gpca_admix.cpp sizes its buffers with and walks the plans of
tests/cpp/admix_plan_audit.cpp's grid of row counts, sample counts and K: the [partial][2] log-likelihood slab of the hold-out step is
written exactly once per entry and read exactly once, inside its capacity; the GPCA_ERR_OOM sum of a hold-out call equals its
allocations; a tile's four philox calls are the global quads of its rows; and the fold of a word is below the fold count with the
boundaries where the rule puts them."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hold_out_extents_fit_and_every_slab_entry_is_written_once(tmp_path):
    exe = str(tmp_path / "admix_cv_plan_audit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "genomic_pca_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "admix_cv_plan_audit.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("admix_cv_plan_audit:") and " 0 failures" in last, last
    assert int(last.split()[1]) > 100_000 and int(last.split()[3]) > 100_000 and int(last.split()[5]) > 10_000, last   # checks; plans; walked
