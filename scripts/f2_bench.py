#!/usr/bin/env python3
"""gpca_f2_blocks on one GPU, in one process: ms per matrix of the library's "group_counts" record (the genotype sweep, k_group_counts)
and of its "f2_blocks" record (k_f2_blocks: the reduction over the counts workspace), added over the row bands of
io.group_count_bands, at 3, 16 and 64 groups on int8 and on 2-bit rows; wall_ms adds the workspace, the uploads and the copy of the
sums.  In the same run, the path the library offered for the same numbers before gpca_f2_blocks: banded gpca_group_counts (its wall
time with the copy of the counts to the host) and gpca_fst_hudson on the host, one call per run of rows of one block so that its sums
fold per block.  That path runs on every --host-sample-th band-sized slice of the rows and is scaled to the matrix; the line says so.
Median and range over the repetitions.

usage: python scripts/f2_bench.py [--rows M] [--samples N] [--groups 3,16,64] [--blocks B] [--storages int8,2bit] [--reps R]
                                  [--host-sample 16] [--out FILE]

The matrix comes from the device generator (six populations); the samples are dealt to the groups round-robin.  One JSON line per
(storage, groups), appended to --out when given."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genomic_pca_amd as g          # noqa: E402
from genomic_pca_amd import _lib     # noqa: E402
from genomic_pca_amd import io as gio  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--samples", type=int, default=10_000)
ap.add_argument("--groups", default="3,16,64")
ap.add_argument("--blocks", type=int, default=600)
ap.add_argument("--storages", default="int8,2bit")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--host-sample", type=int, default=16)
ap.add_argument("--out", default="")
a = ap.parse_args()
M, N = a.rows, a.samples
NAMES = ("group_counts", "f2_blocks")


def stats(v):
    return None if not v else {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def emit(line):
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


def device_path(e, group, P, block, B):
    ms = {k: [] for k in NAMES}
    wall, launches = [], {}
    bands = gio.group_count_bands(M, P, max_rows=gio.F2_BAND_ROWS_MAX)
    e.f2_blocks(group, block[:1024], P, B, rows=(0, min(M, 1024)))                   # warm-up
    for _ in range(a.reps):
        e.reset_timings()
        t0 = time.time()
        acc = np.zeros((B, P * (P - 1) // 2), np.int64)
        cnt = np.zeros_like(acc)
        for r0, r1 in bands:
            ba, bc = e.f2_blocks(group, block[r0:r1], P, B, rows=(r0, r1))
            acc += ba; cnt += bc
        wall.append((time.time() - t0) * 1e3)
        rec = e.timings()
        for k in NAMES:
            ms[k].append(rec[k]["total_ms"])
            launches[k] = rec[k]["launches"]
    return ms, wall, launches, len(bands)


def host_path(e, group, P, block, B):
    """banded gpca_group_counts + gpca_fst_hudson per run of rows of one block, on every host_sample-th slice of each band"""
    pairs = P * (P - 1) // 2
    bands = gio.group_count_bands(M, P)
    t_counts, t_host, rows_done = 0.0, 0.0, 0
    sums = np.zeros((B, max(pairs, 1), 3))
    for r0, r1 in bands:
        n = max((r1 - r0) // a.host_sample, 1)
        t0 = time.time()
        c = e.group_counts(group, P, rows=(r0, r0 + n))
        t_counts += time.time() - t0
        t0 = time.time()
        blk = block[r0:r0 + n]
        cut = np.flatnonzero(np.diff(blk)) + 1
        for s, t in zip(np.r_[0, cut], np.r_[cut, n]):
            g.GpcaEngine.fst_hudson(c[s:t], sums=sums[blk[s]])
        t_host += time.time() - t0
        rows_done += n
    scale = M / rows_done
    return t_counts * 1e3 * scale, t_host * 1e3 * scale, rows_done


for storage in [s for s in a.storages.split(",") if s]:
    store = _lib.STORE_INT8 if storage == "int8" else _lib.STORE_2BIT
    with g.GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=store) as e:
        e.synth_genotypes(M, N, 1, g.synth_thresholds(M, 6, seed=1, fst=0.1))
        e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.ones(M, np.uint8))
        e.enable_timings(True)
        for P in [int(x) for x in a.groups.split(",") if x]:
            group = (np.arange(N) % P).astype(np.int32)
            B = a.blocks
            block = (np.arange(M, dtype=np.int64) * B // M).astype(np.int32)
            ms, wall, launches, nbands = device_path(e, group, P, block, B)
            med = lambda k: float(np.median(ms[k]))
            line = {"bench": "f2_blocks", "matrix": "device generator", "storage": storage, "shape": f"{M} x {N}", "groups": P, "pairs": P * (P - 1) // 2,
                    "blocks": B, "bands": nbands, "reps": a.reps, "group_counts_ms": stats(ms["group_counts"]), "f2_blocks_ms": stats(ms["f2_blocks"]),
                    "wall_ms": stats(wall), "launches_per_matrix": launches,
                    "f2_over_group_counts": round(med("f2_blocks") / med("group_counts"), 3),
                    "f2_counts_gb_s": round(12.0 * M * P / med("f2_blocks") / 1e6, 1)}
            if a.host_sample > 0:
                tc, th, done = host_path(e, group, P, block, B)
                line["host_path"] = {"what": "banded gpca_group_counts (wall, with the copy of the counts) + gpca_fst_hudson per block on the host",
                                     "rows_timed": done, "scaled_by": round(M / done, 2), "group_counts_wall_ms_scaled": round(tc, 1),
                                     "fst_hudson_host_ms_scaled": round(th, 1)}
                line["host_path_over_device_wall"] = round((tc + th) / float(np.median(wall)), 1)
            emit(line)
