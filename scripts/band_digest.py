#!/usr/bin/env python3
"""SHA-256 digests of everything the band calls return (grm, king, pcrelate, pcrelate_isaf, ld_window and their neighbour project), over
a fixed, seeded grid of small cases: evidence that a change to grm.hip / king.hip / pcrelate.hip / ld.hip / project.hip, to their
shared tile helpers or to the host front end of the band calls moves no bit, no exchange and no error text.  Run it on the tree before
and on the tree after the change and diff the two outputs: every line must be equal.  (Not a test: nothing is asserted, and pytest
does not run it.)

usage: python scripts/band_digest.py > digest.txt

One line per case and returned array: storage, N, M, missing rate, the call, the band, the array's name, dtype and shape, the SHA-256 of
its bytes.  The grid is the smallest shapes at which these kernels can go wrong, on int8 and on 2-bit residency:
  N in 63, 65, 127, 129, 257: one below and one above the 64 and the 128 tile edge, and a third tile with one sample;
  M in 31, 33, 65, 4097: a partial block, one row past a 32-row block, past KING's 64-row stage and past GRM's 4 096-row flush group;
  every fifth row is not kept, three calls in a hundred are missing; at M = 65 also no missing call at all (the ballot-off paths);
  grm in both scalings with and without npairs, king with and without counts, pcrelate at P = 0 and 3 with nsnp, pcrelate_isaf,
  ld_window at wmax = 5, project at k = 1 and 33; each on all rows and on the band (tile - 1, tile + 1) where there are that many.
Then grm, king and project on a streamed handle (M = 4097, panels of 8 192 and of 3 072 rows), the three on two ranks through the host
hook (with the element count of every exchange, and with a poisoned genotype on rank 1: status and error text of both ranks), and
the refusals of the five calls as status code and error text.  (The out-of-memory refusals are left out: their text holds the free
memory of the moment.)"""
import hashlib
import os
import sys
import threading

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genomic_pca_amd as g          # noqa: E402
from genomic_pca_amd import _lib     # noqa: E402
from genomic_pca_amd._lib import GpcaError     # noqa: E402

NS = (63, 65, 127, 129, 257)
MS = (31, 33, 65, 4097)
STORES = (("int8", _lib.STORE_INT8), ("2bit", _lib.STORE_2BIT))
WMAX = 5


def inputs(N, M, miss):
    rng = np.random.default_rng(1000 * N + M)
    keep = np.ones(M, np.uint8)
    keep[::5] = 0
    p = rng.uniform(0.1, 0.5, M)
    G = (rng.random((M, N)) < p[:, None]).astype(np.int8) + (rng.random((M, N)) < p[:, None]).astype(np.int8)
    if miss:
        G[rng.random((M, N)) < miss] = -127
    mu = (2 * p).astype(np.float32)
    sigma = np.sqrt(2 * p * (1 - p)).astype(np.float32)
    V = rng.standard_normal((N, 3))
    W = rng.standard_normal((M, 33)).astype(np.float32) * keep[:, None]
    return G, keep, mu, sigma, V, W


def emit(head, res):
    if not isinstance(res, dict):
        res = {str(i): a for i, a in enumerate(res if isinstance(res, tuple) else (res,))}
    for name in sorted(res):
        a = np.ascontiguousarray(res[name])
        print(*head, name, a.dtype.str, "x".join(map(str, a.shape)) or "-", hashlib.sha256(a.tobytes()).hexdigest(), flush=True)


def bands(n, tile):
    return (None, (tile - 1, tile + 1)) if n >= tile + 1 else (None,)


def name_of(rows):
    return "all" if rows is None else f"{rows[0]}:{rows[1]}"


def sample_calls(e, head, N, V, which=("grm", "king", "pcrelate")):
    if "grm" in which:
        for rows in bands(N, 64):
            for sc in ("standardized", "centred"):
                for npairs in (False, True):
                    emit(head + (f"grm-{sc}-np{int(npairs)}", name_of(rows)), e.grm(sc, rows=rows, npairs=npairs))
    if "king" in which:
        for rows in bands(N, 128):
            for counts in (False, True):
                emit(head + (f"king-c{int(counts)}", name_of(rows)), e.king(rows=rows, counts=counts))
    if "pcrelate" in which:
        for rows in bands(N, 128):
            for P in (0, 3):
                emit(head + (f"pcrelate-P{P}", name_of(rows)), e.pcrelate(V[:, :P], rows=rows, nsnp=True))


def row_calls(e, head, V, W, mu, sigma):
    K = e.num_pca_snps()
    for rows in bands(K, 64):
        r0, r1 = (0, K) if rows is None else rows
        we = np.minimum(np.arange(r0, r1) + 1 + WMAX, K)
        emit(head + ("ld", name_of(rows)), e.ld_window(we, wmax=WMAX, rows=rows, threshold=0.2, counts=True))
        emit(head + ("isaf-P3", name_of(rows)), e.pcrelate_isaf(V, rows=rows))
    for k in (1, 33):
        emit(head + (f"project-k{k}", "all"), e.project(mu, sigma, W[:, :k]))


def standardise(e, mu, sigma, keep):
    e.snp_stats(g.QcConfig.none())
    e.set_standardization(mu, sigma, keep)


# 1. the grid on resident handles
for sname, store in STORES:
    for N in NS:
        for M in MS:
            for miss in (0.03, 0.0) if M == 65 else (0.03,):
                G, keep, mu, sigma, V, W = inputs(N, M, miss)
                with g.GpcaEngine(storage=store) as e:
                    e.upload_genotypes_i8(G)
                    standardise(e, mu, sigma, keep)
                    head = (sname, N, M, miss)
                    sample_calls(e, head, N, V)
                    row_calls(e, head, V, W, mu, sigma)

# 2. streamed handles
for sname, store in STORES:
    for N in (65, 257):
        G, keep, mu, sigma, V, W = inputs(N, 4097, 0.03)
        for panel_rows in (8192, 3072):
            with g.GpcaEngine(storage=store) as e:
                e.stream_open(g.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), 4097, N, panel_rows=panel_rows, ring_slots=2, fused=False)
                standardise(e, mu, sigma, keep)
                head = (sname, N, 4097, f"streamed{panel_rows}")
                sample_calls(e, head, N, V, which=("grm", "king"))
                for k in (1, 33):
                    emit(head + (f"project-k{k}", "all"), e.project(mu, sigma, W[:, :k]))


# 3. two ranks through the host hook on one GPU
def two_ranks(G, keep, mu, sigma, call, poison):
    M, world = G.shape[0], 2
    spans = [g.shard_rows(M, world, r) for r in range(world)]
    barrier = threading.Barrier(world, timeout=120)
    bufs, res, counts = [None] * world, [None] * world, [[] for _ in range(world)]

    def run(rank):
        a, b = spans[rank]
        Gr = G[a:b].copy()
        if rank == 1 and poison:
            Gr[np.flatnonzero(keep[a:b])[3], 11] = 3
        with g.GpcaEngine() as e:
            e.upload_genotypes_i8(Gr)

            def hook(buf):
                counts[rank].append(buf.size)
                bufs[rank] = buf.copy(); barrier.wait()
                buf[:] = sum(bufs[r] for r in range(world)); barrier.wait()
            e.set_allreduce_hook(hook, world, rank, a)
            e.set_standardization(mu[a:b], sigma[a:b], keep[a:b])
            try:
                res[rank] = call(e, a, b)
            except GpcaError as err:
                res[rank] = err
    ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in ts]; [t.join() for t in ts]
    return res, counts


N, M = 129, 4097
G, keep, mu, sigma, V, W = inputs(N, M, 0.03)
CALLS = (("grm-standardized", lambda e, a, b: e.grm("standardized", npairs=True)), ("grm-centred-band", lambda e, a, b: e.grm("centred", rows=(63, 65))),
         ("king", lambda e, a, b: e.king(counts=True)), ("king-band", lambda e, a, b: e.king(rows=(127, 129))),
         ("project-k1", lambda e, a, b: e.project(mu[a:b], sigma[a:b], W[a:b, :1])),
         ("project-k33", lambda e, a, b: e.project(mu[a:b], sigma[a:b], W[a:b, :33])))
for cname, call in CALLS:
    for poison in (False, True):
        res, counts = two_ranks(G, keep, mu, sigma, call, poison)
        for rank in range(2):
            head = ("2ranks", N, M, f"poison{int(poison)}", cname, f"rank{rank}")
            print(*head, "exchanges", *counts[rank], flush=True)
            if isinstance(res[rank], GpcaError):
                print(*head, "status", res[rank].status, repr(res[rank].message), flush=True)
            else:
                emit(head, res[rank])


# 4. refusals: status code and error text
def refusal(label, e, fn):
    try:
        rc = fn()
        msg = "" if rc in (None, _lib.GPCA_OK) or not isinstance(rc, int) else _lib.load().gpca_last_error(e._h).decode()
        rc = rc if isinstance(rc, int) else _lib.GPCA_OK
    except GpcaError as err:
        rc, msg = err.status, err.message
    print("refusal", label, rc, repr(msg), flush=True)


lib = _lib.load()
N, M = 129, 65
G, keep, mu, sigma, V, W = inputs(N, M, 0.03)
out = np.empty(N * (N + 1) // 2)
ones = np.ones(M, np.float32)
with g.GpcaEngine() as e:                                              # no genotypes
    refusal("grm-nogeno", e, lambda: lib.gpca_grm(e._h, 0, 0, 1, out.ctypes.data, None))
    refusal("king-nogeno", e, lambda: lib.gpca_king(e._h, 0, 1, out.ctypes.data, None))
    refusal("ld-nogeno", e, lambda: e.ld_window(np.array([1]), wmax=1, rows=(0, 1)))
    refusal("pcrelate-nogeno", e, lambda: lib.gpca_pcrelate(e._h, None, 0, None, 0.01, 0, 1, out.ctypes.data, None))
    refusal("project-nogeno", e, lambda: lib.gpca_project(e._h, mu.ctypes.data, sigma.ctypes.data, W.ctypes.data, 4, out.ctypes.data, None))
with g.GpcaEngine() as e:
    e.upload_genotypes_i8(G)
    refusal("grm-nostats", e, lambda: lib.gpca_grm(e._h, 0, 0, N, out.ctypes.data, None))
    refusal("king-nostats", e, lambda: lib.gpca_king(e._h, 0, N, out.ctypes.data, None))
    refusal("pcrelate-nostats", e, lambda: e.pcrelate(V))
    refusal("ld-nostats", e, lambda: e.ld_window(np.array([1]), wmax=1, rows=(0, 1)))
    standardise(e, mu, sigma, keep)
    K = e.num_pca_snps()
    we = np.minimum(np.arange(K) + 1 + WMAX, K)
    for sc, r0, r1 in ((2, 0, N), (-1, 0, N), (0, -1, N), (0, 5, 5), (0, 10, 3), (0, 0, N + 1)):
        refusal(f"grm-arg-{sc}-{r0}-{r1}", e, lambda: lib.gpca_grm(e._h, sc, r0, r1, out.ctypes.data, None))
    refusal("grm-null", e, lambda: lib.gpca_grm(e._h, 0, 0, N, None, None))
    for r0, r1 in ((-1, N), (5, 5), (10, 3), (0, N + 1)):
        refusal(f"king-arg-{r0}-{r1}", e, lambda: lib.gpca_king(e._h, r0, r1, out.ctypes.data, None))
    refusal("king-null", e, lambda: lib.gpca_king(e._h, 0, N, None, None))
    for r0, r1 in ((-1, K), (10, 3), (0, K + 1)):
        refusal(f"ld-arg-{r0}-{r1}", e, lambda: lib.gpca_ld_window(e._h, r0, r1, we.ctypes.data, WMAX, 0.2, out.ctypes.data, None, None))
    refusal("ld-wmax0", e, lambda: lib.gpca_ld_window(e._h, 0, K, we.ctypes.data, 0, 0.2, out.ctypes.data, None, None))
    refusal("ld-allnull", e, lambda: e.ld_window(we, wmax=WMAX, r2=False))
    for thr in (np.nan, np.inf):
        refusal(f"ld-thr-{thr}", e, lambda: e.ld_window(we, wmax=WMAX, threshold=thr))
    for t, v in ((5, 5), (5, 6 + WMAX + 1), (K - 1, K + 1)):
        bad = we.copy(); bad[t] = v
        refusal(f"ld-winend-{t}-{v}", e, lambda: e.ld_window(bad, wmax=WMAX))
    refusal("pcrelate-P33", e, lambda: e.pcrelate(np.zeros((N, 33))))
    few = np.zeros(N, np.uint8); few[:4] = 1
    refusal("pcrelate-few", e, lambda: e.pcrelate(V, train=few))
    Vc = V.copy(); Vc[:, 2] = 2.0 * Vc[:, 1]
    refusal("pcrelate-collinear", e, lambda: e.pcrelate(Vc))
    refusal("isaf-collinear", e, lambda: e.pcrelate_isaf(Vc))
    Vn = V.copy(); Vn[7, 1] = np.nan
    refusal("pcrelate-nan", e, lambda: e.pcrelate(Vn))
    refusal("pcrelate-tau", e, lambda: e.pcrelate(V, maf_bound=0.5))
    refusal("pcrelate-rows", e, lambda: e.pcrelate(V, rows=(5, N + 1)))
    refusal("pcrelate-null", e, lambda: lib.gpca_pcrelate(e._h, None, 0, None, 0.01, 0, N, None, None))
    refusal("isaf-rows", e, lambda: e.pcrelate_isaf(V, rows=(0, K + 1)))
    for bad_k in (0, 129):
        Wk = np.zeros((M, max(bad_k, 1)), np.float32)
        refusal(f"project-k{bad_k}", e, lambda: lib.gpca_project(e._h, mu.ctypes.data, sigma.ctypes.data, Wk.ctypes.data, bad_k, out.ctypes.data, None))
    for bad_sigma in (np.nan, 0.0):
        s = sigma.copy(); s[2] = bad_sigma
        refusal(f"project-sigma-{bad_sigma}", e, lambda: e.project(mu, s, W[:, :4]))
    for bad_mu, scalings in ((-0.25, (0,)), (np.inf, (0, 1))):
        m2 = mu.copy(); m2[3] = bad_mu
        e.set_standardization(m2, sigma, keep)
        for sc in scalings:
            refusal(f"grm-mu-{bad_mu}-{sc}", e, lambda: lib.gpca_grm(e._h, sc, 0, N, out.ctypes.data, None))
    e.set_standardization(mu, sigma, np.zeros(M, np.uint8))
    refusal("grm-K0", e, lambda: lib.gpca_grm(e._h, 0, 0, N, out.ctypes.data, None))
    refusal("king-K0", e, lambda: lib.gpca_king(e._h, 0, N, out.ctypes.data, None))
    refusal("ld-K0", e, lambda: e.ld_window(we[:0], wmax=WMAX, rows=(0, 0)))
    refusal("pcrelate-K0", e, lambda: e.pcrelate(V))
Gb = G.copy(); Gb[17, 40] = 3
with g.GpcaEngine(storage=_lib.STORE_INT8) as e:
    e.upload_genotypes_i8(Gb)
    standardise(e, ones, ones, np.ones(M, np.uint8))
    K = e.num_pca_snps()
    we = np.minimum(np.arange(K) + 1 + WMAX, K)
    refusal("grm-genotype", e, lambda: e.grm("centred"))
    refusal("king-genotype", e, lambda: e.king())
    refusal("ld-genotype", e, lambda: e.ld_window(we, wmax=WMAX))
    refusal("pcrelate-genotype", e, lambda: e.pcrelate(V))
    refusal("isaf-genotype", e, lambda: e.pcrelate_isaf(V, rows=(0, 4)))
    refusal("project-genotype", e, lambda: e.project(mu, sigma, W[:, :4] + np.float32(1)))
with g.GpcaEngine(precision=_lib.PREC_F32_MFMA) as e:
    e.upload_genotypes_i8(G)
    refusal("project-f32", e, lambda: e.project(mu, sigma, W[:, :4]))
with g.GpcaEngine() as e:                                              # a streamed handle
    e.stream_open(g.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), M, N, panel_rows=128, ring_slots=2, fused=False)
    standardise(e, mu, sigma, keep)
    refusal("pcrelate-streamed", e, lambda: e.pcrelate(V))
    refusal("ld-streamed", e, lambda: e.ld_window(np.array([1]), wmax=1, rows=(0, 1)))
with g.GpcaEngine() as e:                                              # a hooked (row-sharded) handle
    e.upload_genotypes_i8(G)
    e.set_allreduce_hook(lambda buf: None, 2, 0, 0)
    e.set_standardization(mu, sigma, keep)
    refusal("pcrelate-sharded", e, lambda: e.pcrelate(V))
    refusal("ld-sharded", e, lambda: e.ld_window(np.array([1]), wmax=1, rows=(0, 1)))
