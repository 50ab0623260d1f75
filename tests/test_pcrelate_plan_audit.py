"""CPU-only: the extent audit of the PC-Relate host arithmetic (the pcr_* functions of genomic_pca_amd/csrc/plan_math.h).

tests/cpp/pcrelate_plan_audit.cpp includes the header gpca_pcrelate.cpp sizes its launches and buffers with and checks, over a sweep of
(K, N, P) -- kept rows up to 2^31 - 1, samples up to 500 000, every P from 0 to 32 and 300 seeded random values per axis -- that the
grouped and row-major coefficient buffers, the design rows, the hat matrix and the invalid counts hold every index their readers and
writers reach, that the stages and flush groups cover the kept rows once, and that no staged read leaves a row's pitch.  (The band
geometry it shares with GRM and KING: test_band_plan_audit.py.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pcrelate_extents_fit_and_band_is_covered(tmp_path):
    exe = str(tmp_path / "pcrelate_plan_audit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "genomic_pca_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "pcrelate_plan_audit.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("pcrelate_plan_audit:") and " 0 failures" in last, last
    assert int(last.split()[1]) > 100_000, last      # the grid was walked, not skipped
