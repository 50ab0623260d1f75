#!/usr/bin/env python3
"""gpca_king on one GPU: ms per call (HIP events of the library's "king" record: the sweep of per-sample counts and SYRK tiles;
wall_ms adds the kept-row mask, the per-call workspace, the kinship finish and the copy of the band to the host), the int8 MFMA
operations the kernel issues per second on clean blocks (2 x 32^3 per MFMA, 2 MFMAs per 32-row block per 32 x 32 sub-tile of the
128 x 128 tiles on and below the diagonal) as a fraction of the 5 POP/s dense int8 peak, and the genotype bytes of one read of the
matrix per second.  One JSON line.

usage: python scripts/king_bench.py [--rows M] [--samples N] [--storage int8|2bit] [--missing RATE] [--band ROWS] [--reps R]

Clean matrices come from the device generator; with --missing > 0 the rows are a 4 096-row host tile (that missing rate, seeded)
repeated down the matrix and uploaded through a host panel source.  --band ROWS: only rows [0, ROWS) of the triangle (0 = all)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genomic_pca_amd as g          # noqa: E402
from genomic_pca_amd import _lib     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--samples", type=int, default=10_000)
ap.add_argument("--storage", choices=["int8", "2bit"], default="int8")
ap.add_argument("--missing", type=float, default=0.0)
ap.add_argument("--band", type=int, default=0)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
M, N = a.rows, a.samples
band = a.band or N
store = _lib.STORE_INT8 if a.storage == "int8" else _lib.STORE_2BIT
rng = np.random.default_rng(7)

with g.GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=store) as e:
    t0 = time.time()
    if a.missing > 0:
        T = 4096
        th = g.synth_thresholds(T, 6, seed=3, fst=0.1)
        p = th[:, 0].astype(np.float64) / 2**32
        tile = ((rng.random((T, N)) < p[:, None]).astype(np.int8) + (rng.random((T, N)) < p[:, None]).astype(np.int8))
        tile[rng.random((T, N)) < a.missing] = -127
        e.load_from_source(g.PanelSource.host_i8(lambda r0, r: tile[(r0 + np.arange(r)) % T]), M, N)
    else:
        e.synth_genotypes(M, N, 1, g.synth_thresholds(M, 6, seed=1, fst=0.1))
    e.snp_stats()
    load_s = time.time() - t0
    e.king(rows=(0, band))                       # warm-up
    e.enable_timings(True); e.reset_timings()
    t0 = time.time()
    for _ in range(a.reps):
        e.king(rows=(0, band))
    wall_ms = (time.time() - t0) * 1e3 / a.reps
    rec = e.timings().get("king", {})
    ms = rec["total_ms"] / rec["launches"] if rec.get("launches") else float("nan")
    t1 = (band + 127) // 128
    subtiles = 16 * (t1 * (t1 + 1) // 2) - 6 * t1   # 32 x 32 sub-tiles of the 128 x 128 tiles on and below the diagonal
    mpad = (M + 127) // 128 * 128
    ops = 2.0 * 32 ** 3 * 2 * (mpad // 32) * subtiles
    gbytes = M * N / (4 if store == _lib.STORE_2BIT else 1)
    print(json.dumps({"shape": f"{M} x {N}", "band_rows": band, "storage": a.storage, "missing": a.missing,
                      "ms": round(ms, 3), "wall_ms": round(wall_ms, 3), "tops_s": round(ops / ms / 1e9, 1),
                      "frac_5pops": round(ops / ms / 1e9 / 5000.0, 3), "genotype_gb_s": round(gbytes / ms / 1e6, 1),
                      "load_s": round(load_s, 2), "reps": a.reps}))
