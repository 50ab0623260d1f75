#!/usr/bin/env python3
"""gpca_admix_step on one GPU, in one process: ms per EM step of the library's "admix_step" record (HIP events around k_admix_step,
the two slab sums with the F and Q updates and the sum of the log-likelihood terms, without the per-call workspace and the copies) at
K = 3, 8 and 16 on int8 and on 2-bit rows, beside the "sample_counts" record of gpca_sample_counts on the same handle: a kernel that
reads the same rows once and does no arithmetic to speak of.  Median and range over the repetitions.  From the median: the rate of
fused multiply-adds as a21 counts them (6 K per genotype: 2 K for p1 and p0, 2 K for each side) and its share of the f32 vector peak
(157.3 TFLOP/s = 78.65 T multiply-adds per second).

usage: python scripts/admix_bench.py [--rows M] [--samples N] [--ks 3,8,16] [--storages int8,2bit] [--reps R] [--out FILE]

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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default="")
a = ap.parse_args()
M, N = a.rows, a.samples
PEAK_FMA = 157.3e12 / 2
os.environ.pop("GPCA_SAMPLE_COUNTS_SPLITS", None)


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
        e.sample_counts(rows=(0, min(M, 1024)))                                      # warm-up
        for K in [int(k) for k in a.ks.split(",") if k]:
            Q, F = e.admix_init(K, seed=1)
            e.admix_step(Q, F)                                                       # warm-up
            ms, sc, ll = [], [], 0.0
            for _ in range(a.reps):
                e.reset_timings()
                _, _, ll = e.admix_step(Q, F)
                e.sample_counts()
                rec = e.timings()
                ms.append(rec["admix_step"]["total_ms"] / rec["admix_step"]["launches"])
                sc.append(rec["sample_counts"]["total_ms"] / rec["sample_counts"]["launches"])
            med = float(np.median(ms))
            fma = 6.0 * K * M * N / (med * 1e-3)
            emit({"bench": "admix_step", "matrix": "device generator", "storage": storage, "shape": f"{M} x {N}", "K": K, "reps": a.reps,
                  "admix_step_ms": stats(ms), "sample_counts_ms": stats(sc), "step_over_sample_counts": round(med / float(np.median(sc)), 1),
                  "tera_fma_per_s": round(fma / 1e12, 3), "share_of_f32_peak": round(fma / PEAK_FMA, 3), "loglik": ll})
