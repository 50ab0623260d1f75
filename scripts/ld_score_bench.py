#!/usr/bin/env python3
"""gpca_ld_score on one GPU, in one process, beside gpca_ld_window (r2 only) on the same bands: per repetition, the library's "ld" record
(k_ld_vec and k_ld: the banded sweep) and its "ld_score" record (k_ld_score: the planes reduced to one sum per row), both HIP-event times
summed over the bands of io.ld_bands, and the wall time of the whole calls (workspace, memsets, the copy of the results and, for
gpca_ld_window, the 8 B per slot of r2 to the host).  Medians over the repetitions with the smallest and the largest.  One JSON line.

usage: python scripts/ld_score_bench.py [--rows M] [--samples N] [--window W] [--storage int8|2bit] [--reps R]

The matrix comes from the device generator (no missing call); the window is uniform, W slots after every row."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genomic_pca_amd as g          # noqa: E402
from genomic_pca_amd import _lib     # noqa: E402
from genomic_pca_amd import io as gio   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=262_144)
ap.add_argument("--samples", type=int, default=10_000)
ap.add_argument("--window", type=int, default=512)
ap.add_argument("--storage", default="int8")
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()
M, N, W = a.rows, a.samples, a.window
total = lambda rec, name: rec[name]["total_ms"] if rec.get(name, {}).get("launches") else float("nan")


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


with g.GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=_lib.STORE_INT8 if a.storage == "int8" else _lib.STORE_2BIT) as e:
    e.synth_genotypes(M, N, 1, g.synth_thresholds(M, 6, seed=1, fst=0.1))
    e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.ones(M, np.uint8))
    e.enable_timings(True)
    win_end = np.minimum(np.arange(M, dtype=np.int64) + 1 + W, M)
    bands = list(gio.ld_bands(win_end))
    r0, r1, wm = 0, min(M, 1024), max(min(W, M - 1), 1)
    e.ld_score(win_end[r0:r1], wmax=wm, rows=(r0, r1))                      # warm-up of both calls
    e.ld_window(win_end[r0:r1], wmax=wm, rows=(r0, r1))
    score = {"ld_ms": [], "ld_score_ms": [], "wall_ms": []}
    window = {"ld_ms": [], "wall_ms": []}
    acc = None
    for _ in range(a.reps):
        e.reset_timings()
        t0 = time.time()
        parts = [((b0, b1), e.ld_score(win_end[b0:b1], wmax=w, rows=(b0, b1))["score"]) for b0, b1, w in bands]
        score["wall_ms"].append((time.time() - t0) * 1e3)
        rec = e.timings()
        score["ld_ms"].append(total(rec, "ld")); score["ld_score_ms"].append(total(rec, "ld_score"))
        acc = gio.ld_score_sum(M, parts)[0]
        e.reset_timings()
        t0 = time.time()
        for b0, b1, w in bands:
            e.ld_window(win_end[b0:b1], wmax=w, rows=(b0, b1))
        window["wall_ms"].append((time.time() - t0) * 1e3)
        window["ld_ms"].append(total(e.timings(), "ld"))
    l2 = g.GpcaEngine.ld_score_total(acc)
slots = float(sum((b1 - b0) * w for b0, b1, w in bands))
out = {"shape": f"{M} x {N}", "storage": a.storage, "window": W, "bands": len(bands), "slots": slots, "reps": a.reps,
       "gpca_ld_score": {k: stats(v) for k, v in score.items()}, "gpca_ld_window_r2": {k: stats(v) for k, v in window.items()},
       "ld_score_plane_gb_s": round(24.0 * slots / stats(score["ld_score_ms"])["median"] / 1e6, 1), "mean_l2": round(float(l2.mean()), 4)}
print(json.dumps(out))
