#!/usr/bin/env python3
"""gpca_pcrelate on one GPU: ms per call (HIP events of the library's "pcrelate" record: the per-sample invalid counts, the SYRK tiles of
the two products and the finish; "pcrelate_beta": the regression pass; wall_ms adds the host design, the per-call workspace and the
copy of the band to the host), the f32 matrix-core flops per second counted as two products of 2 K pairs flops over the band's entries,
as a fraction of the 157 TF/s f32 MFMA peak, and the genotype bytes of one read of the matrix per second.  One JSON line.

usage: python scripts/pcrelate_bench.py [--rows M] [--samples N] [--storage int8|2bit] [--missing RATE] [--band ROWS] [--pcs P] [--reps R]

Clean matrices come from the device generator; with --missing > 0 the rows are a 4 096-row host tile (that missing rate, seeded)
repeated down the matrix and uploaded through a host panel source.  --band ROWS: only rows [0, ROWS) of the triangle (0 = all).
The coordinates are the population indicator columns of the generator's six populations and random orthonormal columns."""
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
ap.add_argument("--storage", choices=["int8", "2bit"], default="int8")
ap.add_argument("--missing", type=float, default=0.0)
ap.add_argument("--band", type=int, default=0)
ap.add_argument("--pcs", type=int, default=2)
ap.add_argument("--reps", type=int, default=2)
a = ap.parse_args()
M, N, P = a.rows, a.samples, a.pcs
band = a.band or N
store = _lib.STORE_INT8 if a.storage == "int8" else _lib.STORE_2BIT
rng = np.random.default_rng(7)
V = np.linalg.qr(rng.standard_normal((N, max(P, 1))))[0][:, :P]

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
    e.pcrelate(V, rows=(0, min(band, 128)))      # warm-up
    e.enable_timings(True); e.reset_timings()
    t0 = time.time()
    for _ in range(a.reps):
        e.pcrelate(V, rows=(0, band))
    wall_ms = (time.time() - t0) * 1e3 / a.reps
    tm = e.timings()

    def per_launch(name):
        rec = tm.get(name, {})
        return rec["total_ms"] / rec["launches"] if rec.get("launches") else float("nan")
    ms, beta_ms = per_launch("pcrelate"), per_launch("pcrelate_beta")
    pairs = band * (band + 1) // 2
    flops = 2 * 2.0 * K * pairs
    gbytes = M * N / (4 if store == _lib.STORE_2BIT else 1)
    print(json.dumps({"shape": f"{M} x {N}", "kept_rows": K, "band_rows": band, "storage": a.storage, "missing": a.missing, "pcs": P,
                      "ms": round(ms, 3), "pcrelate_beta_ms": round(beta_ms, 3), "wall_ms": round(wall_ms, 3),
                      "f32_tflops": round(flops / ms / 1e9, 2), "frac_157tf": round(flops / ms / 1e9 / 157.0, 3),
                      "genotype_gb_s": round(gbytes / ms / 1e6, 1), "load_s": round(load_s, 2), "reps": a.reps}))
