#!/usr/bin/env python3
"""gpca_group_counts on one GPU: ms per call of the counting kernel (HIP events of the library's "group_counts" record: k_group_counts,
without the one-hot kernel, the per-call workspace and the copy of the counts) for each group count asked for, the genotype bytes per
second that time implies, and beside it the "assoc" record of gpca_assoc_linear with T + Pc = 32 on the same handle (k_assoc: a scan that
also reads every genotype once).  wall_ms adds the labels' upload, the workspace and the copy of the counts to the host.  One JSON line.

usage: python scripts/group_counts_bench.py [--rows M] [--samples N] [--groups P1,P2,...] [--storage int8|2bit] [--missing RATE] [--reps R]
                                            [--no-assoc]

The matrix comes from the device generator (with --missing > 0 a 4 096-row host tile with that missing rate, repeated); the labels are
uniform over the groups, one sample in twenty without a group."""
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
ap.add_argument("--groups", default="2,26,64")
ap.add_argument("--storage", choices=["int8", "2bit"], default="int8")
ap.add_argument("--missing", type=float, default=0.0)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--no-assoc", action="store_true")
a = ap.parse_args()
M, N = a.rows, a.samples
Ps = [int(p) for p in a.groups.split(",")]
store = _lib.STORE_INT8 if a.storage == "int8" else _lib.STORE_2BIT
rng = np.random.default_rng(7)
row_bytes = N / (4 if store == _lib.STORE_2BIT else 1)

with g.GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=store) as e:
    t0 = time.time()
    if a.missing > 0:
        K = 4096
        th = g.synth_thresholds(K, 6, seed=3, fst=0.1)
        p = th[:, 0].astype(np.float64) / 2**32
        tile = ((rng.random((K, N)) < p[:, None]).astype(np.int8) + (rng.random((K, N)) < p[:, None]).astype(np.int8))
        tile[rng.random((K, N)) < a.missing] = -127
        e.load_from_source(g.PanelSource.host_i8(lambda r0, r: tile[(r0 + np.arange(r)) % K]), M, N)
    else:
        e.synth_genotypes(M, N, 1, g.synth_thresholds(M, 6, seed=1, fst=0.1))
    e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.ones(M, np.uint8))
    load_s = time.time() - t0
    e.enable_timings(True)
    per = lambda rec, name: rec[name]["total_ms"] / rec[name]["launches"] if rec.get(name, {}).get("launches") else float("nan")
    out = {"shape": f"{M} x {N}", "storage": a.storage, "missing": a.missing, "reps": a.reps}
    for P in Ps:
        labels = rng.integers(0, P, N).astype(np.int32)
        labels[rng.random(N) < 0.05] = -1
        e.group_counts(labels, P, rows=(0, min(M, 1024)))                    # warm-up
        e.reset_timings()
        t0 = time.time()
        for _ in range(a.reps):
            e.group_counts(labels, P)
        wall_ms = (time.time() - t0) * 1e3 / a.reps
        ms = per(e.timings(), "group_counts")
        out[f"P{P}"] = {"ms": round(ms, 3), "genotype_gb_s": round(M * row_bytes / ms / 1e6, 1), "wall_ms": round(wall_ms, 1)}
    if not a.no_assoc:
        Y = rng.standard_normal((N, 22))
        C = rng.standard_normal((N, 10))
        e.assoc_linear(Y, C, rows=(0, min(M, 1024)))                         # warm-up
        e.reset_timings()
        for _ in range(a.reps):
            e.assoc_linear(Y, C)
        ms = per(e.timings(), "assoc")
        out["assoc_linear_32"] = {"ms": round(ms, 3), "genotype_gb_s": round(M * row_bytes / ms / 1e6, 1)}
    out["load_s"] = round(load_s, 2)
    print(json.dumps(out))
