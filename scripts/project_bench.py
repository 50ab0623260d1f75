#!/usr/bin/env python3
"""gpca_project on one GPU: ms per call (HIP events of the library's "project" record: the sweep and the combine; wall_ms adds the host-side
model scan, the per-call workspace and the uploads) and the genotype bytes
that call streams as a fraction of 8 TB/s.  One JSON line.

usage: python scripts/project_bench.py [--rows M] [--samples N] [--storage int8|2bit] [--k K] [--missing RATE] [--reps R]

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

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--samples", type=int, default=10_000)
ap.add_argument("--storage", choices=["int8", "2bit"], default="int8")
ap.add_argument("--k", type=int, default=20)
ap.add_argument("--missing", type=float, default=0.0)
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()
M, N, k = a.rows, a.samples, a.k
store = _lib.STORE_INT8 if a.storage == "int8" else _lib.STORE_2BIT
rng = np.random.default_rng(7)
mu = rng.uniform(0.1, 1.9, M).astype(np.float32)
sigma = rng.uniform(0.3, 1.0, M).astype(np.float32)
W = (rng.standard_normal((M, k)) * 1e-3).astype(np.float32)

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
    load_s = time.time() - t0
    e.project(mu, sigma, W)                      # warm-up
    e.enable_timings(True); e.reset_timings()
    t0 = time.time()
    for _ in range(a.reps):
        e.project(mu, sigma, W)
    wall_ms = (time.time() - t0) * 1e3 / a.reps
    rec = e.timings().get("project", {})
    ms = rec["total_ms"] / rec["launches"] if rec.get("launches") else float("nan")
    streamed = (M * N / (4 if store == _lib.STORE_2BIT else 1)) * ((k + 31) // 32)
    print(json.dumps({"shape": f"{M} x {N}", "storage": a.storage, "k": k, "missing": a.missing, "ms": round(ms, 3),
                      "wall_ms": round(wall_ms, 3), "bytes": int(streamed), "tb_s": round(streamed / ms / 1e9, 3),
                      "frac_8tbs": round(streamed / ms / 1e9 / 8.0, 3), "load_s": round(load_s, 2), "reps": a.reps}))
