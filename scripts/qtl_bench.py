#!/usr/bin/env python3
"""gpca_assoc_qtl on one GPU, in one process: ms per call of the library's "assoc_qtl" record (k_assoc_qtl and the fold of the bests) and
of its "assoc_qtl_rows" record (the per-row pass on the covariates), the wall time of the call (host design, uploads, the kernels, the
copy and the sort of the hits), and the share of the 157 TF f32 matrix peak that 2 rows N Tpad flops in the "assoc_qtl" time come to.
In the same run, the path the library offered for the same hits before gpca_assoc_qtl: a loop of gpca_assoc_linear calls over trait
groups of 64 - Pc columns with xb and rowinfo copied to the host (no stats table; yy is handed over), r2 formed and thresholded in
numpy.  That loop runs on the first 1 / --loop-sample of the rows and is scaled to the band; the line says so.  Median and range over
the repetitions.

usage: python scripts/qtl_bench.py [--rows M] [--samples 1024,10000] [--traits 1024,8192] [--pcs 10] [--log10p 5]
                                   [--storages int8,2bit] [--reps R] [--loop-sample 16] [--out FILE]

The matrix comes from the device generator; the traits and covariates are standard normal.  One JSON line per (storage, N, T), appended
to --out when given."""
import argparse
import ctypes as C_
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
ap.add_argument("--samples", default="1024,10000")
ap.add_argument("--traits", default="1024,8192")
ap.add_argument("--pcs", type=int, default=10)
ap.add_argument("--log10p", type=float, default=5.0)
ap.add_argument("--storages", default="int8,2bit")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--loop-sample", type=int, default=16)
ap.add_argument("--out", default="")
a = ap.parse_args()
M, Pc = a.rows, a.pcs
PEAK_TF = 157.0
VIF = 50.0


def stats(v):
    return {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def emit(line):
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


def loop_path(e, Y, C, yy, r2_min, rows):
    """the gpca_assoc_linear loop over trait groups on the rows [0, rows), xb and rowinfo copied to the host (no stats table), r2 formed
    and thresholded in numpy: wall seconds and the hits it finds.  yy is handed over (gpca_assoc_linear does not return it)."""
    lib = _lib.load()
    vp = lambda v: v.ctypes.data_as(C_.c_void_p)
    T = Y.shape[1]
    W = 64 - Pc
    t0 = time.time()
    found = 0
    info = np.zeros((rows, 4))
    for c0 in range(0, T, W):
        w = min(W, T - c0)
        Yg = np.ascontiguousarray(Y[:, c0:c0 + w])
        xb = np.zeros((rows, w + Pc))
        rc = lib.gpca_assoc_linear(e._h, vp(Yg), w, vp(C), Pc, None, VIF, 0, rows, None, vp(xb), vp(info))
        assert rc == 0, rc
        xx, sxx = info[:, 2], info[:, 3]
        with np.errstate(all="ignore"):
            live = ~((info[:, 0] == 0) | ~(xx > 0.0) | (sxx * VIF < xx))
            r2 = (xb[:, :w] * xb[:, :w]) / (sxx[:, None] * yy[None, c0:c0 + w])
            found += int((live[:, None] & (r2 >= r2_min)).sum())
    return time.time() - t0, found


for storage in [s for s in a.storages.split(",") if s]:
    store = _lib.STORE_INT8 if storage == "int8" else _lib.STORE_2BIT
    for N in [int(x) for x in a.samples.split(",") if x]:
        with g.GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=store) as e:
            e.synth_genotypes(M, N, 1, g.synth_thresholds(M, 6, seed=1, fst=0.1))
            e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.ones(M, np.uint8))
            e.enable_timings(True)
            rng = np.random.default_rng(1)
            C = rng.standard_normal((N, Pc))
            df = float(N - Pc - 2)
            tmin = g.qtl_t_min(a.log10p, df)
            r2_min = tmin * tmin / (tmin * tmin + df)
            for T in [int(x) for x in a.traits.split(",") if x]:
                Y = rng.standard_normal((N, T))
                e.assoc_qtl(Y[:, :64], C, max_vif=VIF, r2_min=r2_min, rows=(0, min(M, 1024)))      # warm-up
                ms, rows_ms, wall, nf = [], [], [], 0
                for _ in range(a.reps):
                    e.reset_timings()
                    t0 = time.time()
                    q = e.assoc_qtl(Y, C, max_vif=VIF, r2_min=r2_min, cap=1 << 20)
                    wall.append((time.time() - t0) * 1e3)
                    rec = e.timings()
                    ms.append(rec["assoc_qtl"]["total_ms"]); rows_ms.append(rec["assoc_qtl_rows"]["total_ms"])
                    nf = q["n_found"]
                tpad = (T + 63) // 64 * 64
                tf = 2.0 * M * N * tpad / (float(np.median(ms)) * 1e-3) / 1e12
                line = {"bench": "assoc_qtl", "matrix": "device generator", "storage": storage, "shape": f"{M} x {N}", "traits": T, "pcs": Pc,
                        "log10p": a.log10p, "t_min": round(tmin, 4), "hits": nf, "reps": a.reps, "assoc_qtl_ms": stats(ms),
                        "assoc_qtl_rows_ms": stats(rows_ms), "wall_ms": stats(wall), "tflops": round(tf, 1),
                        "share_of_f32_matrix_peak": round(tf / PEAK_TF, 3)}
                if a.loop_sample > 0:
                    rows = max(M // a.loop_sample, 1)
                    sec, found = loop_path(e, Y, C, q["yy"], r2_min, rows)
                    scale = M / rows
                    line["assoc_linear_loop"] = {"what": "gpca_assoc_linear per 64 - Pc traits (wall, with the copy of xb and rowinfo, no stats table) + r2 and threshold in numpy",
                                                 "calls": -(-T // (64 - Pc)), "rows_timed": rows, "scaled_by": round(scale, 2),
                                                 "wall_ms_scaled": round(sec * 1e3 * scale, 1), "hits_in_rows_timed": found}
                    line["loop_over_qtl_wall"] = round(sec * 1e3 * scale / float(np.median(wall)), 2)
                emit(line)
