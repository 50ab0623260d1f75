#!/usr/bin/env python3
"""gpca_ld_window on one GPU, the way the command lines call it: threshold bits only, every kept row, in the row bands of io.ld_bands.
ms = HIP events of the library's "ld" records summed over the bands of one pass (the per-row sums and the banded sweep); wall_ms adds the
per-call workspace, its memset, the finish kernel and the copy of the bits to the host.  genotype_gb_s = one read of the kept rows
per ms; tops_s = int8 MFMA operations on clean blocks (2 x 32^3 per MFMA, one per 32 samples per 32 x 32 tile that meets the band).
One JSON line.

usage: python scripts/ld_bench.py [--rows M] [--samples N] [--storage int8|2bit] [--missing RATE] [--wmax W] [--reps R]

Clean matrices come from the device generator; with --missing > 0 the rows are a 4 096-row host tile (that missing rate, seeded)
repeated down the matrix and uploaded through a host panel source."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genomic_pca_amd as g          # noqa: E402
from genomic_pca_amd import _lib     # noqa: E402
from genomic_pca_amd import io as gio  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--samples", type=int, default=10_000)
ap.add_argument("--storage", choices=["int8", "2bit"], default="int8")
ap.add_argument("--missing", type=float, default=0.0)
ap.add_argument("--wmax", type=int, default=50)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
M, N, W = a.rows, a.samples, a.wmax
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
    K = len(e.pca_snp_rows())
    win_end = np.minimum(np.arange(K, dtype=np.int64) + 1 + W, K)
    bands = list(gio.ld_bands(win_end))

    def one_pass():
        n = 0
        for r0, r1, wm in bands:
            n += int(np.count_nonzero(e.ld_window(win_end[r0:r1], wmax=wm, rows=(r0, r1), threshold=0.2, r2=False)["above"]))
        return n
    one_pass()                                   # warm-up
    e.enable_timings(True); e.reset_timings()
    t0 = time.time()
    for _ in range(a.reps):
        one_pass()
    wall_ms = (time.time() - t0) * 1e3 / a.reps
    rec = e.timings().get("ld", {})
    ms = rec["total_ms"] / a.reps if rec.get("launches") else float("nan")
    tiles = 0
    for r0, r1, wm in bands:                     # per 64-row block: column tiles T with 32 (T - rt) < W + 32 for the two row tiles rt
        tiles += -(-(r1 - r0) // 64) * 2 * ((W + 31) // 32 + 1)
    ops = 2.0 * 32 ** 3 * (-(-N // 32)) * tiles
    gbytes = K * N / (4 if store == _lib.STORE_2BIT else 1)
    print(json.dumps({"shape": f"{M} x {N}", "kept_rows": K, "wmax": W, "bands": len(bands), "storage": a.storage, "missing": a.missing,
                      "ms": round(ms, 3), "wall_ms": round(wall_ms, 3), "tops_s": round(ops / ms / 1e9, 1),
                      "genotype_gb_s": round(gbytes / ms / 1e6, 1), "frac_8tbs": round(gbytes / ms / 1e6 / 8000.0, 3),
                      "load_s": round(load_s, 2), "reps": a.reps}))
