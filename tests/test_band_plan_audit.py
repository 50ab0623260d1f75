"""CPU-only: the audit of the band geometry gpca_grm, gpca_king and gpca_pcrelate share (band_entries, band_index, band_tile_count,
band_tile_list of genomic_pca_amd/csrc/plan_math.h).

tests/cpp/band_plan_audit.cpp includes the header the three entry points and their kernels use and checks, for (tile, diagonal) =
(64, with), (128, without) and (128, with), exhaustively for every N <= 300 and every band 0 <= row0 < row1 <= N, that the tile list
has band_tile_count entries, that every band entry is owned by exactly one (tile, sub-tile not skipped above the diagonal,
accumulator element, lane half), that the indices of the owned entries are a permutation of [0, band_entries) and that no owned
element lies outside the band; then a seeded random sweep of bands at and off the tile edges for up to 500 000 samples.  The
accumulator row map is written out by hand in the audit, not taken from the kernels' header."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_band_is_covered_once_and_indexed_densely(tmp_path):
    exe = str(tmp_path / "band_plan_audit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "genomic_pca_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "band_plan_audit.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("band_plan_audit:") and " 0 failures" in last, last
    assert int(last.split()[1]) > 50_000_000, last      # the grid was walked, not skipped
