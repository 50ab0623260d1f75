"""Tile-edge shapes shared by the gpca_grm, gpca_king and gpca_project modules: sample counts at and around the output tiles (64, 128),
kSamplePad (256) and kSamplePad2bit (1 024), down to one sample; row counts at and around the 32-row block and the flush group of
4 096 rows, down to one row.  Each list walks one axis; tests/_combos.py crosses the axes (sample count x kept rows x keep pattern x
band x storage x missing calls), pairwise, for the band kernels."""
import numpy as np

EDGE_N = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025]
EDGE_M = [1, 31, 32, 33, 4095, 4096, 4097, 8193]


def edge_shapes(n_for_rows):
    """every EDGE_N at 4 097 rows, and every EDGE_M at the two sample counts `n_for_rows`"""
    return [(4097, n) for n in EDGE_N] + [(m, n) for n in n_for_rows for m in EDGE_M]


def edge_keeps(M):
    """(a) one row only, (b) the whole last partial 32-row block dropped (the last full one where M is a multiple of 32; not for
    M <= 32, where nothing would be left), (c) everything.  uint8 masks."""
    one = np.zeros(M, np.uint8); one[M // 2] = 1
    out = [("one row", one), ("every row", np.ones(M, np.uint8))]
    if M > 32:
        tail = np.ones(M, np.uint8); tail[(M - 1) // 32 * 32:] = 0
        out.insert(1, ("last block dropped", tail))
    return out
