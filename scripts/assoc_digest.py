#!/usr/bin/env python3
"""SHA-256 digests of everything the association scans return, over a fixed, seeded grid of small cases: evidence that a change to
the kernels of assoc.hip / assoc_score.hip / assoc_spa.hip, to their shared stage pipeline or to the host front end moves no bit.  Run
it on the tree before and on the tree after the change and diff the two outputs: every line must be equal.  (Not a test: nothing is
asserted, and pytest does not run it.)

usage: python scripts/assoc_digest.py > digest.txt

One line per case and returned array: storage, N, K, the call, T, Pc, the band, the array's name, dtype and shape, the SHA-256 of its
bytes.  The grid is the smallest shapes at which the stage loop can go wrong, on int8 and on 2-bit residency:
  N in 63, 65, 257, 1025: a partial first stage, a second stage with one sample, one sample past a flush group, several flush groups
      with a one-sample tail;
  K in 1, 129: one row, and a second workgroup with a single row (the keep mask has holes: every fifth row of the matrix is dropped);
  assoc_linear (xb=True) at (T, Pc) = (1, 0), (16, 16), (33, 31): panel widths padded to 32, exactly 32, and 64;
  assoc_logistic_score (ua=True), assoc_logistic_spa at spa_z = 2 and at inf, at (T, Pc) = (1, 0), (8, 1), (8, 5): L = 3, 32 and 64;
  every call on all kept rows and, where K > 1, on the band (1, K).
Three calls in a hundred are missing, every tenth sample is excluded.  The inputs depend on N and K alone, so the lines of the two
storages differ in their first field only."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genomic_pca_amd as g          # noqa: E402
from genomic_pca_amd import _lib     # noqa: E402

NS = (63, 65, 257, 1025)
KS = (1, 129)
LINEAR = ((1, 0), (16, 16), (33, 31))
LOGISTIC = ((1, 0), (8, 1), (8, 5))
STORES = (("int8", _lib.STORE_INT8), ("2bit", _lib.STORE_2BIT))


def inputs(N, K):
    rng = np.random.default_rng(1000 * N + K)
    kept = np.arange(K) * 5 // 4 + 1                      # rows 0, 5, 10, ... are holes, and so is the last row
    M = int(kept[-1]) + 2
    keep = np.zeros(M, np.uint8)
    keep[kept] = 1
    p = rng.uniform(0.1, 0.9, M)[:, None]
    G = (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)
    G[rng.random((M, N)) < 0.03] = -127
    inc = np.ones(N, np.uint8)
    inc[5::10] = 0
    C = rng.standard_normal((N, 31))
    Y = rng.standard_normal((N, 33)) + 0.3 * C[:, :1]
    Yb = (rng.random((N, 8)) < 1.0 / (1.0 + np.exp(-0.5 * C[:, :1]))).astype(np.float64)
    return G, keep, inc, C, Y, Yb


def emit(head, res):
    for name in sorted(res):
        a = np.ascontiguousarray(res[name])
        print(*head, name, a.dtype.str, "x".join(map(str, a.shape)) or "-", hashlib.sha256(a.tobytes()).hexdigest(), flush=True)


for sname, store in STORES:
    for N in NS:
        for K in KS:
            G, keep, inc, C, Y, Yb = inputs(N, K)
            with g.GpcaEngine(storage=store) as e:
                e.upload_genotypes_i8(G)
                M = G.shape[0]
                e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), keep)
                for rows in (None, (1, K)) if K > 1 else (None,):
                    band = "all" if rows is None else f"{rows[0]}:{rows[1]}"
                    for T, Pc in LINEAR:
                        emit((sname, N, K, "linear", T, Pc, band), e.assoc_linear(Y[:, :T], C[:, :Pc], inc, rows=rows, xb=True))
                    for T, Pc in LOGISTIC:
                        emit((sname, N, K, "score", T, Pc, band), e.assoc_logistic_score(Yb[:, :T], C[:, :Pc], inc, rows=rows, ua=True))
                        for z in (2.0, float("inf")):
                            emit((sname, N, K, f"spa{z:g}", T, Pc, band),
                                 e.assoc_logistic_spa(Yb[:, :T], C[:, :Pc], inc, spa_z=z, rows=rows, ua=True))
