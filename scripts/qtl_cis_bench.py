#!/usr/bin/env python3
"""gpca_assoc_qtl_cis on one GPU, in one process: ms per call of the library's "qtl_perm_panel" record (k_qtl_perm_panel, summed over the
traits), of its "assoc_qtl_cis" record (k_assoc_qtl_cis and the fold of the bests, summed over the traits) and the wall time of the call
(host design, the upload of the table, the per-row pass, the kernels, one copy of the results).
In the same run, the path the library offered before gpca_assoc_qtl_cis: per trait, the permuted columns built and projected in numpy
(residual, gather through the table, the covariates taken out again), then one gpca_assoc_qtl call over the trait's window with the P + 1
columns as traits and best=True.  That loop runs on the first --loop-traits traits, once to warm up and then --reps times, and its
median is scaled to all traits; the line says so.  Median and range over the repetitions.

usage: python scripts/qtl_cis_bench.py [--rows M] [--samples 1024] [--windows 2048,8192] [--perms 1000,10000] [--traits 64] [--pcs 10]
                                       [--storages int8,2bit] [--reps R] [--loop-traits 2] [--out FILE]

The matrix comes from the device generator; the traits and covariates are standard normal; trait g's window starts at
g (M - window) / (traits - 1).  One JSON line per (storage, N, window, P), appended to --out when given."""
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
ap.add_argument("--rows", type=int, default=65536)
ap.add_argument("--samples", default="1024")
ap.add_argument("--windows", default="2048,8192")
ap.add_argument("--perms", default="1000,10000")
ap.add_argument("--traits", type=int, default=64)
ap.add_argument("--pcs", type=int, default=10)
ap.add_argument("--storages", default="int8,2bit")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--loop-traits", type=int, default=2)
ap.add_argument("--out", default="")
a = ap.parse_args()
M, Pc, G = a.rows, a.pcs, a.traits
VIF = 50.0


def stats(v):
    return {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def emit(line):
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


def loop_path(e, Y, C, win, perm, traits):
    """per trait: residual, permuted columns and their projection in numpy, then gpca_assoc_qtl over the window with the P + 1 columns
    as traits: wall seconds"""
    t0 = time.time()
    Cc = C - C.mean(0)
    Q, _ = np.linalg.qr(Cc / np.sqrt((Cc ** 2).sum(0)))
    for t in range(traits):
        y = Y[:, t] - Y[:, t].mean()
        b = y - Q @ (Q.T @ y)
        V = b[perm].T                                                  # [N][P]
        V = V - Q @ (Q.T @ V)
        Yp = np.ascontiguousarray(np.hstack([b[:, None], V]))
        e.assoc_qtl(Yp, C, max_vif=VIF, r2_min=1.0, cap=0, rows=(int(win[t, 0]), int(win[t, 1])))
    return time.time() - t0


for storage in [s for s in a.storages.split(",") if s]:
    store = _lib.STORE_INT8 if storage == "int8" else _lib.STORE_2BIT
    for N in [int(x) for x in a.samples.split(",") if x]:
        with g.GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=store) as e:
            e.synth_genotypes(M, N, 1, g.synth_thresholds(M, 6, seed=1, fst=0.1))
            e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.ones(M, np.uint8))
            e.enable_timings(True)
            rng = np.random.default_rng(1)
            C = rng.standard_normal((N, Pc))
            Y = rng.standard_normal((N, G))
            for W in [int(x) for x in a.windows.split(",") if x]:
                lo = (np.arange(G) * (M - W) // max(G - 1, 1)).astype(np.int64)
                win = np.stack([lo, lo + W], 1)
                for P in [int(x) for x in a.perms.split(",") if x]:
                    perm = g.qtl_perm_table(1, N, P)
                    e.assoc_qtl_cis(Y[:, :2], win[:2], C, max_vif=VIF, perm=perm[:8])          # warm-up
                    panel_ms, scan_ms, wall = [], [], []
                    for _ in range(a.reps):
                        e.reset_timings()
                        t0 = time.time()
                        q = e.assoc_qtl_cis(Y, win, C, max_vif=VIF, perm=perm)
                        wall.append((time.time() - t0) * 1e3)
                        rec = e.timings()
                        panel_ms.append(rec["qtl_perm_panel"]["total_ms"]); scan_ms.append(rec["assoc_qtl_cis"]["total_ms"])
                    tpad = (P + 1 + 63) // 64 * 64
                    tf = 2.0 * G * W * N * tpad / (float(np.median(scan_ms)) * 1e-3) / 1e12
                    line = {"bench": "assoc_qtl_cis", "matrix": "device generator", "storage": storage, "shape": f"{M} x {N}", "traits": G,
                            "window_rows": W, "perms": P, "pcs": Pc, "reps": a.reps, "qtl_perm_panel_ms": stats(panel_ms),
                            "assoc_qtl_cis_ms": stats(scan_ms), "wall_ms": stats(wall), "scan_tflops": round(tf, 1),
                            "min_n_var": int(q["n_var"].min())}
                    if a.loop_traits > 0:
                        nt = min(a.loop_traits, G)
                        loop_path(e, Y, C, win, perm, 1)                                           # warm-up
                        loop = [loop_path(e, Y, C, win, perm, nt) * 1e3 * G / nt for _ in range(a.reps)]
                        line["assoc_qtl_loop"] = {"what": "per trait: permuted columns built and projected in numpy, one gpca_assoc_qtl call over the window (wall)",
                                                  "traits_timed": nt, "scaled_by": round(G / nt, 2), "wall_ms_scaled": stats(loop)}
                        line["loop_over_cis_wall"] = round(float(np.median(loop)) / float(np.median(wall)), 2)
                    emit(line)
