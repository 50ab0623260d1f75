#!/usr/bin/env python3
"""gpca_assoc_linear on one GPU: ms per call (HIP events of the library's "assoc" record: the k_assoc pass over the band; wall_ms adds
the host design, the per-call workspace, the finish kernel and the copy of the outputs to the host), the f32 matrix-core flops per
second counted as 2 K N L_pad (the d product; the e product runs only where calls are missing), as a fraction of the 157 TF/s f32
MFMA peak, and the genotype bytes of one read of the band per second beside the 8 TB/s of the HBM.  One JSON line per L.

usage: python scripts/assoc_bench.py [--rows M] [--samples N] [--storage int8|2bit] [--missing RATE] [--cols L ...] [--band ROWS] [--reps R]
                                     [--score] [--spa] [--firth]

Clean matrices come from the device generator; with --missing > 0 the rows are a 4 096-row host tile (that missing rate, seeded)
repeated down the matrix and uploaded through a host panel source.  --band ROWS: rows per call (0 = io.assoc_bands' default).  Of the
L columns a third (at most 20) are covariates: random orthonormal columns; the traits are standard normal.

--score: gpca_assoc_logistic_score beside gpca_assoc_linear at the same panel width in the same run (k_assoc is the yardstick): per L
(32 = 8 traits x (1 covariate + 3), 64 = 16 x 4; any other L is taken as T = L // 4 traits with one covariate) one JSON line with
"assoc_score" ms (the k_assoc_score pass), "assoc_score_count" ms (the count sweep that decides the flip), "assoc" ms at the same L and
the ratio (score + count) / assoc; wall_ms adds the null fits on the host.  The traits are Bernoulli(0.4), the covariate standard
normal.

--spa (with the shapes of --score): gpca_assoc_logistic_spa beside gpca_assoc_logistic_score on the same traits in the same run, the
three calls alternating rep by rep: per L one JSON line with the wall ms of a pass over the bands for the score call, for the new call
at spa_z = inf (nothing corrected: the flag kernel and the copy of its output are all it adds) and at spa_z = 2, each as the median
of the reps with the smallest and largest beside it, the "assoc_spa" ms of the library's record (the flag and correction kernels) at
either cutoff, and the share of the items with status >= 1 at spa_z = 2.  The traits are Bernoulli(0.1) here: the unbalanced case the
correction exists for.

--firth (with the shapes and traits of --spa): gpca_assoc_logistic_firth at firth_z = inf and at 1.959964 beside the score call and the
saddle-point call at spa_z = 2 on the same traits in the same run, the four calls alternating rep by rep: the wall ms of each as
median, smallest and largest, the "assoc_firth" ms of the library's record at either cutoff, the share of the items corrected and the
count of items with status 2."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genomic_pca_amd as g          # noqa: E402
from genomic_pca_amd import _lib, io as gio     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--samples", type=int, default=10_000)
ap.add_argument("--storage", choices=["int8", "2bit"], default="int8")
ap.add_argument("--missing", type=float, default=0.0)
ap.add_argument("--cols", type=int, nargs="+", default=[32, 64])
ap.add_argument("--band", type=int, default=0)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--score", action="store_true")
ap.add_argument("--spa", action="store_true")
ap.add_argument("--firth", action="store_true")
a = ap.parse_args()
M, N = a.rows, a.samples
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
    K = e.num_pca_snps()
    load_s = time.time() - t0
    for L in a.cols if a.spa else []:
        T, Pc = max(L // 4, 1), 1
        Yb = (rng.random((N, T)) < 0.1).astype(np.float64)
        Cs = rng.standard_normal((N, Pc))
        bands = [(r0, min(r0 + a.band, K)) for r0 in range(0, K, a.band)] if a.band else gio.assoc_score_bands(K, T, Pc)
        calls = {"score": lambda b: e.assoc_logistic_score(Yb, Cs, rows=b), "spa_inf": lambda b: e.assoc_logistic_spa(Yb, Cs, spa_z=float("inf"), rows=b),
                 "spa_2": lambda b: e.assoc_logistic_spa(Yb, Cs, spa_z=2.0, rows=b)}
        for f in calls.values():
            f((0, min(K, 128)))                          # warm-up
        e.enable_timings(True)
        wall, spa_ms, flagged, items = {k: [] for k in calls}, {}, 0, 0
        for r in range(a.reps):
            for k, f in calls.items():
                e.reset_timings()
                t0 = time.time()
                for b in bands:
                    res = f(b)
                    if k == "spa_2" and r == 0:
                        flagged += int((res["spa_status"] >= 1).sum()); items += res["spa_status"].size
                wall[k].append((time.time() - t0) * 1e3)
                spa_ms[k] = e.timings().get("assoc_spa", {}).get("total_ms", float("nan"))
        stat = lambda v: [round(float(np.median(v)), 3), round(min(v), 3), round(max(v), 3)]
        print(json.dumps({"shape": f"{M} x {N}", "kept_rows": K, "storage": a.storage, "missing": a.missing, "L": T * (Pc + 3), "traits": T,
                          "covariates": Pc, "bands": len(bands), "score_wall_ms_med_min_max": stat(wall["score"]),
                          "spa_inf_wall_ms_med_min_max": stat(wall["spa_inf"]), "spa_2_wall_ms_med_min_max": stat(wall["spa_2"]),
                          "assoc_spa_ms_at_inf": round(spa_ms["spa_inf"], 3), "assoc_spa_ms_at_2": round(spa_ms["spa_2"], 3),
                          "flagged_share_at_2": round(flagged / max(items, 1), 5), "load_s": round(load_s, 2), "reps": a.reps}), flush=True)
    for L in a.cols if a.firth else []:
        T, Pc = max(L // 4, 1), 1
        Yb = (rng.random((N, T)) < 0.1).astype(np.float64)
        Cs = rng.standard_normal((N, Pc))
        bands = [(r0, min(r0 + a.band, K)) for r0 in range(0, K, a.band)] if a.band else gio.assoc_score_bands(K, T, Pc)
        inf = float("inf")
        calls = {"score": lambda b: e.assoc_logistic_score(Yb, Cs, rows=b), "spa_2": lambda b: e.assoc_logistic_spa(Yb, Cs, spa_z=2.0, rows=b),
                 "firth_inf": lambda b: e.assoc_logistic_firth(Yb, Cs, firth_z=inf, rows=b),
                 "firth_196": lambda b: e.assoc_logistic_firth(Yb, Cs, firth_z=1.959964, rows=b)}
        for f in calls.values():
            f((0, min(K, 128)))                          # warm-up
        e.enable_timings(True)
        wall, rec_ms, status = {k: [] for k in calls}, {}, []
        for r in range(a.reps):
            for k, f in calls.items():
                e.reset_timings()
                t0 = time.time()
                for b in bands:
                    res = f(b)
                    if k == "firth_196" and r == 0:
                        status.append(res["firth_status"].ravel().copy())
                wall[k].append((time.time() - t0) * 1e3)
                rec_ms[k] = e.timings().get("assoc_firth", {}).get("total_ms", float("nan"))
        st = np.concatenate(status)
        stat = lambda v: [round(float(np.median(v)), 3), round(min(v), 3), round(max(v), 3)]
        print(json.dumps({"shape": f"{M} x {N}", "kept_rows": K, "storage": a.storage, "missing": a.missing, "L": T * (Pc + 3), "traits": T,
                          "covariates": Pc, "bands": len(bands), "score_wall_ms_med_min_max": stat(wall["score"]),
                          "spa_2_wall_ms_med_min_max": stat(wall["spa_2"]), "firth_inf_wall_ms_med_min_max": stat(wall["firth_inf"]),
                          "firth_1.959964_wall_ms_med_min_max": stat(wall["firth_196"]), "assoc_firth_ms_at_inf": round(rec_ms["firth_inf"], 3),
                          "assoc_firth_ms_at_1.959964": round(rec_ms["firth_196"], 3), "corrected_share": round(float((st == 1).mean()), 5),
                          "failed": int((st == 2).sum()), "load_s": round(load_s, 2), "reps": a.reps}), flush=True)
    for L in a.cols if a.score and not a.spa and not a.firth else []:
        T, Pc = max(L // 4, 1), 1
        Ls = T * (Pc + 3)
        Yb = (rng.random((N, T)) < 0.4).astype(np.float64)
        Cs = rng.standard_normal((N, Pc))
        Yl = rng.standard_normal((N, Ls - Pc))
        bands = [(r0, min(r0 + a.band, K)) for r0 in range(0, K, a.band)] if a.band else gio.assoc_score_bands(K, T, Pc)
        e.assoc_logistic_score(Yb, Cs, rows=(0, min(K, 128))); e.assoc_linear(Yl, Cs, rows=(0, min(K, 128)))      # warm-up
        e.enable_timings(True); e.reset_timings()
        t0 = time.time()
        for _ in range(a.reps):
            for b in bands:
                e.assoc_logistic_score(Yb, Cs, rows=b)
        wall_ms = (time.time() - t0) * 1e3 / a.reps
        for _ in range(a.reps):
            for b in bands:
                e.assoc_linear(Yl, Cs, rows=b)
        tm = e.timings()
        ms = {k: (tm[k]["total_ms"] / a.reps if tm.get(k, {}).get("launches") else float("nan")) for k in ("assoc_score", "assoc_score_count", "assoc")}
        lpad = 32 if Ls <= 32 else 64
        gbytes = K * N / (4 if store == _lib.STORE_2BIT else 1)
        print(json.dumps({"shape": f"{M} x {N}", "kept_rows": K, "storage": a.storage, "missing": a.missing, "L": Ls, "traits": T, "covariates": Pc,
                          "bands": len(bands), "assoc_score_ms": round(ms["assoc_score"], 3), "assoc_score_count_ms": round(ms["assoc_score_count"], 3),
                          "assoc_ms_same_L": round(ms["assoc"], 3), "ratio_to_assoc": round((ms["assoc_score"] + ms["assoc_score_count"]) / ms["assoc"], 3),
                          "issued_multiplies_ratio": round((8 * lpad / 32 + 8) / (8 * lpad / 32), 3), "wall_ms": round(wall_ms, 3),
                          "read_at_8tbs_ms": round(gbytes / 8e12 * 1e3, 3), "mfma_at_157tf_ms": round(2.0 * K * N * (lpad + 32) / 157e12 * 1e3, 3),
                          "load_s": round(load_s, 2), "reps": a.reps}), flush=True)
    for L in [] if a.score or a.spa or a.firth else a.cols:
        Pc = min(L // 3, 20)
        Y = rng.standard_normal((N, L - Pc))
        C = np.linalg.qr(rng.standard_normal((N, max(Pc, 1))))[0][:, :Pc]
        bands = [(r0, min(r0 + a.band, K)) for r0 in range(0, K, a.band)] if a.band else gio.assoc_bands(K, L)
        e.assoc_linear(Y, C, rows=(0, min(K, 128)))      # warm-up
        e.enable_timings(True); e.reset_timings()
        t0 = time.time()
        for _ in range(a.reps):
            for b in bands:
                e.assoc_linear(Y, C, rows=b)
        wall_ms = (time.time() - t0) * 1e3 / a.reps
        rec = e.timings().get("assoc", {})
        ms = rec["total_ms"] / a.reps if rec.get("launches") else float("nan")
        lpad = 32 if L <= 32 else 64
        flops = 2.0 * K * N * lpad
        gbytes = K * N / (4 if store == _lib.STORE_2BIT else 1)
        read_ms, mfma_ms = gbytes / 8e12 * 1e3, flops / 157e12 * 1e3
        print(json.dumps({"shape": f"{M} x {N}", "kept_rows": K, "storage": a.storage, "missing": a.missing, "L": L, "traits": L - Pc, "covariates": Pc,
                          "bands": len(bands), "ms": round(ms, 3), "wall_ms": round(wall_ms, 3), "read_at_8tbs_ms": round(read_ms, 3),
                          "mfma_at_157tf_ms": round(mfma_ms, 3), "frac_of_larger_bound": round(max(read_ms, mfma_ms) / ms, 3),
                          "f32_tflops": round(flops / ms / 1e9, 2), "genotype_gb_s": round(gbytes / ms / 1e6, 1), "load_s": round(load_s, 2),
                          "reps": a.reps}), flush=True)
