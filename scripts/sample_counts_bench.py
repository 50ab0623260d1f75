#!/usr/bin/env python3
"""gpca_sample_counts on one GPU, in one process: ms per call of the counting pass (HIP events of the library's "sample_counts" record:
k_sample_counts and k_sc_sum, without the per-call workspace, the weights' upload and the copy of the sums) on int8 and on 2-bit rows,
without and with weights, the genotype bytes per second that time implies and their fraction of the HBM peak; beside it the
"group_counts" record of gpca_group_counts with P groups on the same handle (a kernel that reads the same bytes), and one run on a
matrix with missing calls.  wall_ms adds the workspace, the upload and the copies.  One JSON line.

usage: python scripts/sample_counts_bench.py [--rows M] [--samples N] [--groups P] [--storages int8,2bit] [--splits S1,S2,...]
                                             [--missing RATE] [--missing-rows M2] [--reps R] [--hbm-tb-s X]

The matrix comes from the device generator; the weights are uniform over 0 .. 2^30.  --splits also times the forced split counts
(GPCA_SAMPLE_COUNTS_SPLITS) beside the default plan.  With --missing > 0 a further int8 matrix of M2 rows is loaded from a 4 096-row host
tile with that missing rate, repeated."""
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
ap.add_argument("--groups", type=int, default=26)
ap.add_argument("--storages", default="int8,2bit")
ap.add_argument("--splits", default="")
ap.add_argument("--missing", type=float, default=0.02)
ap.add_argument("--missing-rows", type=int, default=262_144)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--hbm-tb-s", type=float, default=8.0)
a = ap.parse_args()
M, N = a.rows, a.samples
rng = np.random.default_rng(7)
per = lambda rec, name: rec[name]["total_ms"] / rec[name]["launches"] if rec.get(name, {}).get("launches") else float("nan")
os.environ.pop("GPCA_SAMPLE_COUNTS_SPLITS", None)


def fig(ms, rows, row_bytes):
    gbs = rows * row_bytes / ms / 1e6
    return {"ms": round(ms, 3), "genotype_gb_s": round(gbs, 1), "hbm_fraction": round(gbs / (a.hbm_tb_s * 1e3), 3)}


def time_sample_counts(e, rows, row_bytes, q):
    e.sample_counts(None if q is None else q[:min(rows, 1024)], rows=(0, min(rows, 1024)))      # warm-up
    e.reset_timings()
    t0 = time.time()
    for _ in range(a.reps):
        e.sample_counts(q)
    wall = (time.time() - t0) * 1e3 / a.reps
    r = fig(per(e.timings(), "sample_counts"), rows, row_bytes)
    r["wall_ms"] = round(wall, 1)
    return r


out = {"shape": f"{M} x {N}", "reps": a.reps, "hbm_tb_s": a.hbm_tb_s}
for storage in a.storages.split(","):
    store = _lib.STORE_INT8 if storage == "int8" else _lib.STORE_2BIT
    row_bytes = N / (4 if store == _lib.STORE_2BIT else 1)
    with g.GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=store) as e:
        e.synth_genotypes(M, N, 1, g.synth_thresholds(M, 6, seed=1, fst=0.1))
        e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.ones(M, np.uint8))
        e.enable_timings(True)
        q = rng.integers(0, (1 << 30) + 1, M).astype(np.uint32)
        res = {"counts": time_sample_counts(e, M, row_bytes, None), "counts_q": time_sample_counts(e, M, row_bytes, q)}
        for s in [int(x) for x in a.splits.split(",") if x]:
            os.environ["GPCA_SAMPLE_COUNTS_SPLITS"] = str(s)                      # (read per call)
            res[f"splits{s}"] = {"counts": time_sample_counts(e, M, row_bytes, None)["ms"], "counts_q": time_sample_counts(e, M, row_bytes, q)["ms"]}
            os.environ.pop("GPCA_SAMPLE_COUNTS_SPLITS")
        labels = rng.integers(0, a.groups, N).astype(np.int32)
        e.group_counts(labels, a.groups, rows=(0, min(M, 1024)))                 # warm-up
        e.reset_timings()
        for _ in range(a.reps):
            e.group_counts(labels, a.groups)
        res[f"group_counts_P{a.groups}"] = fig(per(e.timings(), "group_counts"), M, row_bytes)
        out[storage] = res
if a.missing > 0:
    K, M2 = 4096, a.missing_rows
    th = g.synth_thresholds(K, 6, seed=3, fst=0.1)
    p = th[:, 0].astype(np.float64) / 2**32
    tile = ((rng.random((K, N)) < p[:, None]).astype(np.int8) + (rng.random((K, N)) < p[:, None]).astype(np.int8))
    tile[rng.random((K, N)) < a.missing] = -127
    with g.GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=_lib.STORE_INT8) as e:
        e.load_from_source(g.PanelSource.host_i8(lambda r0, r: tile[(r0 + np.arange(r)) % K]), M2, N)
        e.set_standardization(np.ones(M2, np.float32), np.ones(M2, np.float32), np.ones(M2, np.uint8))
        e.enable_timings(True)
        q = rng.integers(0, (1 << 30) + 1, M2).astype(np.uint32)
        out[f"int8_missing_{a.missing:g}"] = {"shape": f"{M2} x {N}", "counts": time_sample_counts(e, M2, N, None),
                                              "counts_q": time_sample_counts(e, M2, N, q)}
print(json.dumps(out))
