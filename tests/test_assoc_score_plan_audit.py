"""CPU-only: the extent audit of the logistic score scan's host arithmetic (the asr_* functions of genomic_pca_amd/csrc/plan_math.h).

tests/cpp/assoc_score_plan_audit.cpp includes the header gpca_assoc_score.cpp sizes its launches and buffers with and checks, over a
sweep of (N, T, Pc, K, band) -- samples up to 2^30 - 1, every (T, Pc) the call accepts and with them every L from 3 to 64, kept rows
up to 2^31 - 1, bands at the tile edges and 300 seeded random values per axis -- that the panel's columns are laid out once with every
w column in the first block of 32, that the panel, the include words, dv, the per-row sums, stats, ua and rowinfo hold every index
their readers and writers reach, that the count kernel's chunks cover the samples once inside a row's pitch, and that the workgroups
of the count kernel and of the scan cover a band's rows once."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_assoc_score_extents_fit_and_band_is_covered(tmp_path):
    exe = str(tmp_path / "assoc_score_plan_audit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "genomic_pca_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "assoc_score_plan_audit.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("assoc_score_plan_audit:") and " 0 failures" in last, last
    assert int(last.split()[1]) > 100_000, last      # the grid was walked, not skipped
