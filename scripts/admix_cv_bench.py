#!/usr/bin/env python3
"""gpca_admix_step_holdout beside gpca_admix_step on one GPU, in one process: ms per step of the library's "admix_step_holdout" and
"admix_step" records (HIP events around the four launches of a step, without the per-call workspace and the copies) at K = 3, 8 and 16
on int8 and on 2-bit rows, v folds, fold 0.  What the hold-out costs beside 6 K multiply-adds, two divisions and two logf per call: four
philox4x32-10 calls per thread and tile of 16 rows, a second f64 register and two counters.  Median and range over the repetitions.

usage: python scripts/admix_cv_bench.py [--rows M] [--samples N] [--ks 3,8,16] [--storages int8,2bit] [--folds V] [--reps R] [--out FILE]

The matrix comes from the device generator; Q and F are gpca_admix_init's.  One JSON line per storage and K, appended to --out when
given."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genomic_pca_amd as g          # noqa: E402
from genomic_pca_amd import _lib     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--samples", type=int, default=10_000)
ap.add_argument("--ks", default="3,8,16")
ap.add_argument("--storages", default="int8,2bit")
ap.add_argument("--folds", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default="")
a = ap.parse_args()
M, N, V = a.rows, a.samples, a.folds


def stats(v):
    return {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def emit(line):
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


for storage in [s for s in a.storages.split(",") if s]:
    store = _lib.STORE_INT8 if storage == "int8" else _lib.STORE_2BIT
    with g.GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=store) as e:
        e.synth_genotypes(M, N, 1, g.synth_thresholds(M, 6, seed=1, fst=0.1))
        e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.ones(M, np.uint8))
        e.enable_timings(True)
        for K in [int(k) for k in a.ks.split(",") if k]:
            Q, F = e.admix_init(K, seed=1)
            e.admix_step(Q, F); e.admix_step_holdout(Q, F, V, 0)                     # warm-up
            plain, held, r = [], [], {}
            for _ in range(a.reps):
                e.reset_timings()
                e.admix_step(Q, F)
                r = e.admix_step_holdout(Q, F, V, 0)
                rec = e.timings()
                plain.append(rec["admix_step"]["total_ms"] / rec["admix_step"]["launches"])
                held.append(rec["admix_step_holdout"]["total_ms"] / rec["admix_step_holdout"]["launches"])
            emit({"bench": "admix_step_holdout", "matrix": "device generator", "storage": storage, "shape": f"{M} x {N}", "K": K, "folds": V,
                  "reps": a.reps, "admix_step_ms": stats(plain), "admix_step_holdout_ms": stats(held),
                  "holdout_over_step": round(float(np.median(held)) / float(np.median(plain)), 3), "n_held": r["n_held"],
                  "held_loglik": r["held_loglik"]})
