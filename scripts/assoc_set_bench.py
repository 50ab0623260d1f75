#!/usr/bin/env python3
"""gpca_assoc_logistic_set on one GPU: ms per call of the Gram of the sets' scores (HIP events of the library's "assoc_set_gram" record:
k_assoc_set_gram and its finish kernel) beside the score scan of the same listed rows inside the same call ("assoc_score_count" +
"assoc_score"), their ratio, the f32 multiply-adds of the XX product per second and the genotype bytes the Gram reads per second
(a strip stages its set's rows once per trait).  wall_ms adds the null fits on the host, the per-call workspace and the copies.
One JSON line.

usage: python scripts/assoc_set_bench.py [--sets S] [--set-rows M] [--samples N] [--traits T] [--covariates P] [--storage int8|2bit]
                                         [--missing RATE] [--reps R]

The matrix holds S x M rows from the device generator (with --missing > 0 a 4 096-row host tile with that missing rate, repeated); set s
lists the rows [s M, (s + 1) M)."""
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
ap.add_argument("--sets", type=int, default=1000)
ap.add_argument("--set-rows", type=int, default=64)
ap.add_argument("--samples", type=int, default=100_000)
ap.add_argument("--traits", type=int, default=1)
ap.add_argument("--covariates", type=int, default=10)
ap.add_argument("--storage", choices=["int8", "2bit"], default="int8")
ap.add_argument("--missing", type=float, default=0.0)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
S, m, N, T, Pc = a.sets, a.set_rows, a.samples, a.traits, a.covariates
M = S * m
store = _lib.STORE_INT8 if a.storage == "int8" else _lib.STORE_2BIT
rng = np.random.default_rng(7)
C = rng.standard_normal((N, Pc))
Y = (rng.random((N, T)) < 1.0 / (1.0 + np.exp(-(0.5 * C[:, :1] - 1.0)))).astype(np.float64) if Pc else (rng.random((N, T)) < 0.3).astype(np.float64)
sets = [np.arange(s * m, (s + 1) * m, dtype=np.int64) for s in range(S)]

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
    e.assoc_logistic_set(Y, sets[:2], C)                                     # warm-up
    e.enable_timings(True); e.reset_timings()
    t0 = time.time()
    for _ in range(a.reps):
        e.assoc_logistic_set(Y, sets, C)
    wall_ms = (time.time() - t0) * 1e3 / a.reps
    rec = e.timings()
    per = lambda name: rec[name]["total_ms"] / rec[name]["launches"] if rec.get(name, {}).get("launches") else float("nan")
    gram, score = per("assoc_set_gram"), per("assoc_score_count") + per("assoc_score")
    tiles = sum(k + 1 for k in range((m + 31) // 32))                        # 32 x 32 tiles of a set's lower triangle
    fma = 2.0 * 32 * 32 * tiles * S * T * N
    staged = sum(min(32 * (k + 1), m) for k in range((m + 31) // 32)) * S * T * N / (4 if store == _lib.STORE_2BIT else 1)
    print(json.dumps({"shape": f"{S} sets x {m} rows, N = {N}, T = {T}, Pc = {Pc}", "storage": a.storage, "missing": a.missing,
                      "gram_ms": round(gram, 3), "score_ms": round(score, 3), "gram_over_score": round(gram / score, 3),
                      "wall_ms": round(wall_ms, 1), "gram_tflops": round(fma / gram / 1e9, 2), "gram_genotype_gb_s": round(staged / gram / 1e6, 1),
                      "load_s": round(load_s, 2), "reps": a.reps}))
