#!/usr/bin/env python3
"""gpca_roh on one GPU, in one process: ms per call of the library's "roh" record (HIP events around k_roh_mark, the count pass of
k_roh_runs and k_roh_stitch, without the per-call workspace and the copies), of its two parts "roh_mark" and "roh_count" and of the fill
pass "roh_fill", on int8 and on 2-bit rows with the default parameters (window 50, 1 het, 5 missing, threshold 1/20, 100 SNPs), beside
the "sample_counts" record of gpca_sample_counts on the same handle: a kernel that reads the same band once with the same access
pattern, so the ratio says what the second read of the window's leaving row and the run pass cost.  Median and range over the
repetitions.  wall_ms adds the workspace, the uploads and the copies (and the wrapper's second call where the first buffer was short).

usage: python scripts/roh_bench.py [--rows M] [--samples N] [--domains D] [--storages int8,2bit] [--het RATE] [--tract-rows M2] [--reps R]
                                   [--out FILE]

The matrix comes from the device generator: independent calls at population frequencies, which hold almost no run at a window of 50.
With --het > 0 a further int8 matrix of M2 rows is loaded from a 4 096-row host tile with that het rate (and the same missing rate),
repeated down the matrix, to time the passes with runs present.  One JSON line per matrix, appended to --out when given."""
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
ap.add_argument("--domains", type=int, default=22)
ap.add_argument("--storages", default="int8,2bit")
ap.add_argument("--het", type=float, default=0.005)
ap.add_argument("--tract-rows", type=int, default=262_144)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default="")
a = ap.parse_args()
N = a.samples
rng = np.random.default_rng(7)
os.environ.pop("GPCA_ROH_SPLITS", None)
os.environ.pop("GPCA_SAMPLE_COUNTS_SPLITS", None)
NAMES = ("roh", "roh_mark", "roh_count", "roh_fill", "sample_counts")


def brk_of(rows):
    b = np.zeros(rows, np.uint8)
    b[(np.arange(a.domains, dtype=np.int64) * rows) // a.domains] = 3
    return b


def stats(v):
    return None if not v else {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def measure(e, rows, row_bytes):
    brk = brk_of(rows)
    e.roh(brk[:1024], rows=(0, min(rows, 1024)))                                     # warm-up
    e.sample_counts(rows=(0, min(rows, 1024)))
    ms = {k: [] for k in NAMES}
    wall, launches, nseg = [], {}, 0
    for _ in range(a.reps):
        e.reset_timings()
        t0 = time.time()
        segs, _count = e.roh(brk)
        wall.append((time.time() - t0) * 1e3)
        e.sample_counts()
        rec = e.timings()
        nseg = int(segs.shape[0])
        for k in NAMES:
            if rec.get(k, {}).get("launches"):
                ms[k].append(rec[k]["total_ms"] / rec[k]["launches"])
                launches[k] = rec[k]["launches"]
    out = {k + "_ms": stats(ms[k]) for k in NAMES}
    out["roh_wall_ms"] = stats(wall)
    out["records"] = nseg
    out["launches_per_call"] = launches
    med = lambda k: float(np.median(ms[k])) if ms[k] else float("nan")
    out["roh_over_sample_counts"] = round(med("roh") / med("sample_counts"), 2)
    out["mark_over_sample_counts"] = round(med("roh_mark") / med("sample_counts"), 2)
    out["mark_genotype_gb_s"] = round(rows * row_bytes / med("roh_mark") / 1e6, 1)       # the band once per pass, whatever the pass re-reads
    return out


def emit(line):
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


M = a.rows
for storage in [s for s in a.storages.split(",") if s]:
    store = _lib.STORE_INT8 if storage == "int8" else _lib.STORE_2BIT
    with g.GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=store) as e:
        e.synth_genotypes(M, N, 1, g.synth_thresholds(M, 6, seed=1, fst=0.1))
        e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.ones(M, np.uint8))
        e.enable_timings(True)
        line = {"bench": "roh", "matrix": "device generator", "storage": storage, "shape": f"{M} x {N}", "domains": a.domains, "reps": a.reps}
        line.update(measure(e, M, N / (4 if store == _lib.STORE_2BIT else 1)))
        emit(line)
if a.het > 0:
    K, M2 = 4096, a.tract_rows
    u = rng.random((K, N))
    tile = np.where(rng.random((K, N)) < 0.5, 0, 2).astype(np.int8)
    tile[u < a.het] = 1
    tile[(u >= a.het) & (u < 2 * a.het)] = -127
    with g.GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=_lib.STORE_INT8) as e:
        e.load_from_source(g.PanelSource.host_i8(lambda r0, r: tile[(r0 + np.arange(r)) % K]), M2, N)
        e.set_standardization(np.ones(M2, np.float32), np.ones(M2, np.float32), np.ones(M2, np.uint8))
        e.enable_timings(True)
        line = {"bench": "roh", "matrix": f"host tile, het {a.het:g}, missing {a.het:g}", "storage": "int8", "shape": f"{M2} x {N}",
                "domains": a.domains, "reps": a.reps}
        line.update(measure(e, M2, N))
        emit(line)
