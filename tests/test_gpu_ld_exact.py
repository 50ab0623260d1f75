"""gpca_ld_window held to its exact integer model (ld.hip, gpca_ld.cpp) at every edge of its launch plan.

THE MODEL.  ``ld_model(G, keep, win_end, wmax, row0, row1)`` restates include/gpca.h section a10 from the genotypes alone.  X = the kept
rows in order; o = [call observed], g' = g on an observed call and 0 on a missing one, q = g'^2.  For band row i = row0 + t and slot d,
j = i + 1 + d, and where j < win_end[t]
    n = sum o_i o_j,  sx = sum g'_i o_j,  sy = sum o_i g'_j,  sxx = sum q_i o_j,  syy = sum o_i q_j,  sxy = sum g'_i g'_j      (int64)
    cov = n sxy - sx sy,  vx = n sxx - sx sx,  vy = n syy - sy sy,  r2 = (cov cov) / (vx vy),  NaN when vx <= 0 or vy <= 0     (f64)
in the order of k_ld_finish; a slot outside the row's window is 0 in r2, in all six counts and in its ``above`` bit, and ``above`` is
r2 > threshold packed little-endian into ceil(wmax / 64) words.  The sums go through f64 matrix products of blocks of rows (every
partial sum is an integer of at most 4 N < 2^53, so any summation order gives the same value) and are converted to int64;
test_model_equals_python_ints checks them against plain Python integers and, on one input, against ``ref_ld`` of test_gpu_ld.py, whose
sums go through f32 products.  The model does not know the device's decomposition (six product planes and three per-row sums); the
mutants do.

THE BAR.  test_every_case_is_in_the_exact_regime asserts that each of n sxy, sx sy, n sxx, sx^2, n syy, sy^2 is below 2^53 in every
device case.  The three differences are then exact whether or not the compiler contracts them into an fma; cov^2, vx vy and the quotient
round once each, as numpy's do.  The device output is therefore a function of the inputs alone, and EVERY device comparison in this
module is np.array_equal (equal_nan for r2) on counts, r2 and the above-words.  There is no tolerance anywhere.

THE PLAN.  ``ld_plan(rows, weff, N)`` restates ld_row_blocks, ld_col_tiles, ld_col_chunks, ld_stages, ld_stages_per_split and
ld_splits of plan_math.h; test_plan_mirror_equals_the_header compares it with what tests/cpp/ld_plan_audit.cpp prints from the header
itself, for every (rows, weff, N) of this module and 200 seeded others.  test_every_plan_regime_is_covered asserts that the device
cases (``every_call``: the one list the device tests, the exact-regime test and the teeth all walk) contain: plain stores with 1, 2 and
>= 3 stages; atomics with 1, 2 and >= 3 stages per split and one with a short last split; 1, 2 and >= 3 column chunks; weff on both
sides of 32|33, 64|65 and 192|193; K in {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129}; bands with row0 % 64 in {0, 1, 63}; a band below
K whose windows reach past row1; N % 16 in {0, 1, 15} and N % 128 in {0, 1, 127}; wmax in {63, 64, 65, 256, 257}.

INPUTS (seeded, ``make_input``).  M = K + 40 rows of which K are kept, scattered (krows is not the identity), or the three masks of
edge_keeps(170) (K = 1, 160, 170).  Each row copies the row before it on 70 % of the samples (LD by construction); with K >= 12 kept
row K // 3 is constant (NaN across its window) and kept rows K // 2 and K // 2 + 1 are equal (r2 = 1 exactly).  Missing patterns:
``none``; ``random`` (2 %, the default of the shape families); ``lonely`` -- one missing call in the whole matrix, at kept row in {0,
31, 32, 63, 64, last} x sample in {0, 15, 16, 127, 128, N - 1}, aimed at the wave ballot, at saw_missing under plain stores (the call
lies in a stage other than the first), at the tail mask and at the aliased chunk 0; ``sided`` -- kept row a is 2 wherever row a + 1 is
missing (and row b + 1 is 2 wherever row b is missing), which separates sxx from sx and the two sides from each other.
Families of calls:
  edges      N in {129, 385} x K in {1, .., 129, 260} and the edge_keeps masks: windows min(i + 1 + w, K), w in {1, 32, 33, 64, 65, 192,
             193} with wmax = w and w + 3 (widths beyond K included), and one ragged win_end (random widths, two chromosome ends).
             K = 260 is there so that w = 192 | 193 are on both sides of the third column chunk.
  bands      K = 260: row0 in {1, 63, 64}, bands that end below K with windows past row1, one-row bands, wmax in {63, 256, 257}
  samples    N in EDGE_N + {383, 384, 385} at K = 130, w = 65
  switch     one handle, K = 8 300, N = 385, w = 1000: the band (0, 7 232) makes 113 x 9 = 1 017 workgroups (atomic, two splits of two
             stages), the band (0, 7 233) 1 026 (plain stores, four stages); both equal the model and their common rows are
             bit-identical.  Every missing pattern; ``last`` of lonely is row 8 232 here, the last row a window of either band reaches.
  thin       K = 32 968, N = 200, w = 65: 32 768 rows make 1 024 workgroups (plain stores, two stages), 32 704 rows 1 022 (atomic)
  split3     16 448 rows, w = 65, N = 600: 514 workgroups, five stages in splits of 3 + 2
  missing    the four patterns at (K, N) = (33, 129), (65, 385), (129, 385), w in {33, 65}
  threshold  two attained r2 values (1.0 and the largest below it) passed as the threshold: above is strictly greater
  subsets    the seven non-empty subsets of {r2, counts, above} through the C ABI, each output bit-equal to the all-three call's
and, outside the list (they return an error, not numbers), all 252 byte values outside {0, 1, 2, 0x81} in int8 storage.

TEETH (CPU).  ``MUTANTS`` are changes of the model, most of them written in the device's decomposition: pad samples counted in n (the
tail mask dropped), the sides swapped (g'm <-> mg'), g' for g'^2 against a missing call, j <= win_end, the last slot of the widest window
dropped, the last sample stage dropped, the last split dropped, kept rows from the last multiple of 32 below K read as zero on the column
side, >= for the threshold, counts left non-zero outside the window, and -- for the rule that a wave which met no missing call leaves the
five extra planes to the memset -- saw_missing taken from the first sample stage only under plain stores.  test_teeth asserts that each moves at least one compared bit in at
least one call of every family it can touch; CANNOT_TOUCH lists, with the reason, the families it cannot, and they are asserted to be
untouched.  (Calls of more than 512 rows are bitten on their first 128 rows, their last 128 and the 128 around the rows of ``sided``,
with the launch plan of the whole call; the model is separable by row.)  ``vx < 0 for vx <= 0`` is not a mutant: vx = 0 means the
row is constant over the jointly observed samples, so cov = 0 too, the quotient is 0 / 0 and it is NaN either way.

RECORDS (not thresholds; each test prints its own with -s).  On one MI355X the 163 device cases of this module take 19 s, the models
included: 1 432 calls (716 per storage) and 4 422 comparisons of counts, r2 or above-words with the model or with another call, every
one of them bit-equal, and 255 calls that are refused and name the right row.  Of the 1 306 launches of k_ld (the other calls have no
pair in any window), 34 run plain stores with four stages, 2 with two, 28 with one; 34 run atomics with two stages per split, 2 with
splits of 3 + 2, the others with one.  The largest product of the exact-regime test is 2^20.66 (K = 130, N = 1 024), 32 binary orders
below the bar.  The 5 CPU tests take 65 s on 8 cores (the 716 models and the teeth most of it).  Nothing was found wrong in ld.hip
or gpca_ld.cpp.
"""
import math
import os
import subprocess
from collections import namedtuple

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from _edges import EDGE_N, edge_keeps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISSING = -127
STORES = {"int8": _lib.STORE_INT8, "2bit": _lib.STORE_2BIT}
THR = 0.2 + 2.0 ** -30                              # (no small ratio of integers rounds to it: the >= mutant cannot move a bit by accident)
RECORD = {"calls": 0, "comparisons": 0}

Plan = namedtuple("Plan", "workgroups chunks stages per splits kind")
Inp = namedtuple("Inp", "K N keep miss")            # keep: "scattered" or a name of edge_keeps(EDGE_KEEP_M)
Call = namedtuple("Call", "family inp win w wmax band thr")   # win: "count" or "ragged"; thr: a float, "one" or "below one"
Model = namedtuple("Model", "r2 counts inwin")


# ---------------------------------------------------------------------------------------------------------------------------------
# the launch plan, restated
# ---------------------------------------------------------------------------------------------------------------------------------
def ld_plan(rows, weff, N):
    """(workgroups, column chunks, sample stages, stages per split, splits, "plain" | "atomic") of launch_ld"""
    cdiv = lambda a, b: -(-a // b)
    nrb = cdiv(rows, 64)
    tiles = (64 - 1 + weff) // 32 + 1
    nch = cdiv(tiles, 4)
    nst = cdiv(N, 128)
    nb = nrb * nch
    S = 1 if nb >= 1024 else cdiv(1024, max(nb, 1))
    S = max(min(S, nst), 1)
    per = cdiv(nst, S)
    splits = cdiv(nst, per)
    return Plan(nb, nch, nst, per, splits, "atomic" if splits > 1 else "plain")


# ---------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------
def _band_products(pairs, K, row0, row1, wmax):
    """for each (A, B) of `pairs` ([K][n] f64 matrices of small integers): int64 [rows][wmax], slot (t, d) = sum_n A[i, n] B[j, n] with
    i = row0 + t, j = i + 1 + d; 0 where j >= K"""
    rows = row1 - row0
    out = [np.zeros((rows, wmax), np.int64) for _ in pairs]
    d = np.arange(wmax)
    B = 256
    for b0 in range(row0, row1, B):
        b1 = min(b0 + B, row1)
        c1 = min(b1 + wmax, K)                      # columns b0 + 1 .. c1 - 1
        if c1 <= b0 + 1:
            continue
        t = np.arange(b1 - b0)
        col = t[:, None] + d[None, :]               # column index j - (b0 + 1)
        ok = col < c1 - (b0 + 1)
        colc = np.where(ok, col, 0)
        for o, (L, R) in zip(out, pairs):
            P = L[b0:b1] @ R[b0 + 1:c1].T
            assert P.max(initial=0.0) < 2.0 ** 53
            o[b0 - row0:b1 - row0] = np.where(ok, P[t[:, None], colc], 0.0).astype(np.int64)
    return out


def _operands(X, cols=None):
    X = X if cols is None else X[:, cols]
    o = X != MISSING
    g = np.where(o, X, 0).astype(np.float64)
    return g, g * g, o.astype(np.float64), (~o).astype(np.float64)


def finish(cnt, inwin, counts_outside=False):
    """r2 in the order of k_ld_finish from int64 counts [rows][wmax][6]; both are zeroed outside the window"""
    c = cnt.astype(np.float64)
    n, sx, sy, sxx, syy, sxy = (c[..., s] for s in range(6))
    cov, vx, vy = n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy
    with np.errstate(divide="ignore", invalid="ignore"):
        r2 = (cov * cov) / (vx * vy)
    r2[(vx <= 0.0) | (vy <= 0.0)] = np.nan
    r2[~inwin] = 0.0
    if not counts_outside:
        cnt[~inwin] = 0
    return r2


def ld_model(G, keep, win_end, wmax, row0=0, row1=None, mut=None, plan=None, weff=None):
    """Model(r2 f64 [rows][wmax], counts int32 [rows][wmax][6], inwin) of kept rows [row0, row1); win_end has one entry per band row.
    mut: a name of MUTANTS, with the launch plan and the widest window of the call it stands in for (teeth only)."""
    X = np.asarray(G)[np.asarray(keep).astype(bool)]
    K, N = X.shape
    row1 = K if row1 is None else row1
    rows = row1 - row0
    we = np.asarray(win_end, np.int64)
    assert we.shape == (rows,)
    if rows > 1024 and mut is None:                  # (the model is separable by row: large bands in pieces, to bound the temporaries)
        parts = [ld_model(G, keep, we[a - row0:min(a + 1024, row1) - row0], wmax, a, min(a + 1024, row1)) for a in range(row0, row1, 1024)]
        return Model(*(np.concatenate([p[k] for p in parts]) for k in range(3)))
    assert np.all((X == MISSING) | ((X >= 0) & (X <= 2))), "a kept row holds an invalid call"
    X = X[row0:min(K, row1 + wmax)]                  # the rows the band reads; the products below index them from row0
    g, q, o, m = _operands(X)
    bp = lambda pairs: _band_products(pairs, X.shape[0], 0, rows, wmax)
    cnt = np.stack(bp([(o, o), (g, o), (o, g), (q, o), (o, q), (g, g)]), axis=-1)
    j = np.arange(row0, row1)[:, None] + 1 + np.arange(wmax)[None, :]
    inwin = (j <= we[:, None]) if mut == "j <= win_end" else (j < we[:, None])
    if mut in PLANE_MUTANTS:
        # the device's decomposition: n = N - miss_i - miss_j + mm, sx = sum g'_i - g'm, sy = sum g'_j - mg', sxx = sum q_i - qm,
        # syy = sum q_j - mq, sxy = g'g'; a plane that loses the part D of its sum moves its count by -+ D
        if mut in ("last stage dropped", "last split dropped"):
            first = 128 * (plan.stages - 1) if mut == "last stage dropped" else 128 * plan.per * (plan.splits - 1)
            if mut == "last split dropped" and plan.splits == 1:
                first = N                            # (plain stores have one split: nothing to drop)
            gD, qD, oD, mD = _operands(X, slice(first, N))
            xy, gm, mg, qm, mq, mm = bp([(gD, gD), (gD, mD), (mD, gD), (qD, mD), (mD, qD), (mD, mD)])
            cnt += np.stack([-mm, gm, mg, qm, mq, -xy], axis=-1)
        elif mut == "column tail read as zero":
            xy, gm, mg, qm, mq, mm = bp([(g, g), (g, m), (m, g), (q, m), (m, q), (m, m)])
            lost = (j >= (K - 1) // 32 * 32)[..., None]
            cnt += np.where(lost, np.stack([-mm, gm, mg, qm, mq, -xy], axis=-1), 0)
        elif mut == "sides swapped":
            gm, mg = bp([(g, m), (m, g)])
            cnt[..., 1] += gm - mg; cnt[..., 2] += mg - gm
        elif mut == "g' for g'^2 against a missing call":
            gm, mg, qm, mq = bp([(g, m), (m, g), (q, m), (m, q)])
            cnt[..., 3] += qm - gm; cnt[..., 4] += mq - mg
        elif mut == "saw_missing from the first stage only" and plan.kind == "plain":
            # under plain stores the five extra planes of a pair are left to the memset unless a missing call was seen; seen only in
            # the first stage, a pair whose rows hold their missing calls in later stages loses them
            gm, mg, qm, mq, mm = bp([(g, m), (m, g), (q, m), (m, q), (m, m)])
            seen = np.append(m[:, :128].any(axis=1), False)
            jl = np.minimum(np.arange(rows)[:, None] + 1 + np.arange(wmax)[None, :], X.shape[0])
            lost = ~(seen[:rows][:, None] | seen[jl])[..., None]
            cnt += np.where(lost, np.stack([-mm, gm, mg, qm, mq, 0 * mm], axis=-1), 0)
    if mut == "pad samples counted in n":
        cnt[..., 0] += (-N) % 16
    if mut == "last slot of the widest window dropped":
        inwin = inwin & (np.arange(wmax)[None, :] != weff - 1)
    r2 = finish(cnt, inwin, counts_outside=mut == "counts left outside the window")
    assert np.abs(cnt).max(initial=0) < 2 ** 31
    return Model(r2, cnt.astype(np.int32), inwin)


def above_words(r2, inwin, thr, ge=False):
    """r2 > thr inside the window, packed little-endian into ceil(wmax / 64) uint64 words per row"""
    with np.errstate(invalid="ignore"):
        bits = ((r2 >= thr) if ge else (r2 > thr)) & inwin
    nw = (r2.shape[1] + 63) // 64
    pad = np.zeros((r2.shape[0], nw * 64), bool)
    pad[:, :r2.shape[1]] = bits
    return np.packbits(pad, axis=1, bitorder="little").view("<u8")


def ld_model_python_ints(G, keep, win_end, wmax, row0, row1):
    """the six counts with plain Python integers and loops (small shapes only): [rows][wmax][6]"""
    X = [[int(v) for v in row] for row, k in zip(np.asarray(G), keep) if k]
    K, N = len(X), len(X[0])
    out = [[[0] * 6 for _ in range(wmax)] for _ in range(row1 - row0)]
    for t, i in enumerate(range(row0, row1)):
        for d in range(wmax):
            jj = i + 1 + d
            if jj >= int(win_end[t]) or jj >= K:
                continue
            c = out[t][d]
            for a, b in zip(X[i], X[jj]):
                oa, ob = int(a != MISSING), int(b != MISSING)
                ga, gb = a * oa, b * ob
                c[0] += oa * ob; c[1] += ga * ob; c[2] += oa * gb; c[3] += ga * ga * ob; c[4] += oa * gb * gb; c[5] += ga * gb
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and the list of calls
# ---------------------------------------------------------------------------------------------------------------------------------
K_EDGES = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129]
K_WIDE = 260                                        # w = 192 | 193 on both sides of the third column chunk
W_EDGES = [1, 32, 33, 64, 65, 192, 193]
EDGE_KEEP_M = 170
SAMPLE_EDGES = EDGE_N + [383, 384, 385]
SWITCH = dict(K=8300, N=385, w=1000, atomic=(0, 7232), plain=(0, 7233))
THIN = dict(K=32768 + 200, N=200, w=65, wmax=68, atomic=(0, 32704), plain=(0, 32768))
SPLIT3 = dict(K=16448 + 200, N=600, w=65, wmax=68, band=(0, 16448))
MISSING_SHAPES = [(33, 129), (65, 385), (129, 385)]
_INPUTS = {}


def lonely_rows(K, last=None):
    return sorted({r for r in (0, 31, 32, 63, 64) if r < K} | {K - 1 if last is None else last})


def lonely_samples(N):
    return sorted({s for s in (0, 15, 16, 127, 128) if s < N} | {N - 1})


def keep_mask(inp):
    """uint8 [M]: K ones scattered over K + 40 rows, or a mask of edge_keeps(EDGE_KEEP_M)"""
    if inp.keep != "scattered":
        keep = dict(edge_keeps(EDGE_KEEP_M))[inp.keep]
        assert int(keep.sum()) == inp.K
        return keep
    M = inp.K + 40
    keep = np.zeros(M, np.uint8)
    keep[np.random.default_rng([11, inp.K]).choice(M, inp.K, replace=False)] = 1
    return keep


def make_input(inp):
    """(G int8 [M][N], keep uint8 [M]).  The genotypes of every missing pattern of a shape differ only in the calls the pattern sets.
    Cached; do not modify."""
    if inp in _INPUTS:
        return _INPUTS[inp]
    K, N = inp.K, inp.N
    keep = keep_mask(inp)
    M = keep.size
    kr = np.flatnonzero(keep)
    rng = np.random.default_rng([7, K, N, M])
    p = rng.uniform(0.05, 0.5, size=(M, 1))
    G = (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)
    cp = rng.random((M, N)) < 0.7
    for i in range(1, M):
        if i % 7:
            G[i, cp[i]] = G[i - 1, cp[i]]
    if K >= 12:
        G[kr[K // 3]] = 1                                               # constant: NaN across its window and in the windows that hold it
        G[kr[K // 2]] = (np.arange(N) % 3).astype(np.int8)              # two equal rows next to each other: r2 = 1 exactly (N >= 2)
        G[kr[K // 2 + 1]] = G[kr[K // 2]]
    mrng = np.random.default_rng([13, K, N])
    miss = inp.miss
    if miss == "random":
        G[mrng.random((M, N)) < 0.02] = MISSING
    elif miss == "sided":
        a, b = K // 4, K // 4 + 3
        for lo, hi in ((a + 1, a), (b, b + 1)):                          # (the row with the missing calls, the row that is 2 there)
            at = mrng.random(N) < 0.25
            at[N // 2] = True
            G[kr[lo], at] = MISSING; G[kr[hi], at] = 2
    elif miss != "none":
        assert miss[0] == "lonely"
        G[kr[miss[1]], miss[2]] = MISSING
    G.setflags(write=False); keep.setflags(write=False)
    _INPUTS[inp] = (G, keep)
    return _INPUTS[inp]


def win_end_of(call):
    """win_end [K] of the call's whole handle (the band takes its slice)"""
    K, w = call.inp.K, call.w
    i = np.arange(K, dtype=np.int64)
    if call.win == "count":
        return np.minimum(i + 1 + w, K)
    rng = np.random.default_rng([17, K, w])
    width = rng.integers(0, w + 1, size=K)
    if K:
        width[rng.integers(0, K)] = w                                   # (the widest window is attained)
    ends = np.array(sorted({K // 3, 2 * K // 3, K}) , np.int64)         # two chromosome ends and the end of the rows
    ends = ends[ends > 0]
    chrom_end = ends[np.searchsorted(ends, i, side="right")]
    return np.minimum(i + 1 + width, chrom_end)


def band_weff(call):
    r0, r1 = call.band
    we = win_end_of(call)[r0:r1]
    return int(np.max(we - np.arange(r0, r1) - 1)) if r1 > r0 else 0


def plan_of(call):
    return ld_plan(call.band[1] - call.band[0], band_weff(call), call.inp.N)


def _edge_inputs(N):
    out = [Inp(K, N, "scattered", "random") for K in K_EDGES + [K_WIDE]]
    return out + [Inp(int(k.sum()), N, name, "random") for name, k in edge_keeps(EDGE_KEEP_M)]


def edge_calls(inp):
    K = inp.K
    out = [Call("edges", inp, "count", w, wmax, (0, K), THR) for w in W_EDGES for wmax in (w, w + 3)]
    return out + [Call("edges", inp, "ragged", 70, 73, (0, K), THR)]


def band_calls():
    inp = Inp(K_WIDE, 385, "scattered", "random")
    K = inp.K
    out = [Call("bands", inp, "count", 65, 65, b, THR) for b in ((1, 200), (63, 130), (64, 129), (0, 1), (K - 1, K), (127, 128))]
    out += [Call("bands", inp, "ragged", 70, 73, b, THR) for b in ((1, 200), (63, K))]
    out += [Call("bands", inp, "count", 60, 63, (0, K), THR), Call("bands", inp, "count", 193, 256, (0, K), THR),
            Call("bands", inp, "count", 193, 257, (0, K), THR), Call("bands", inp, "count", 193, 257, (63, 200), THR)]
    return out


def sample_calls(N):
    inp = Inp(130, N, "scattered", "random")
    return [Call("samples", inp, "count", 65, 65, (0, 130), THR), Call("samples", inp, "count", 65, 68, (0, 130), THR)]


SWITCH_LAST = SWITCH["plain"][1] - 1 + SWITCH["w"]                      # 8 232: the last row a window of either band reaches
# (row, sample) of the lonely call at the switch shape: every row of the list, each with one sample in the first stage or in the
# masked tail and, for rows 0 .. 63 and the last, one in a later stage
SWITCH_LONELY = [(0, 16), (31, 127), (32, 128), (63, 384), (64, 0), (SWITCH_LAST, 15),
                 (0, 128), (31, 384), (32, 0), (63, 15), (64, 16), (SWITCH_LAST, 127), (63, 128), (SWITCH_LAST, 384)]
SWITCH_MISS = ["none", "random", "sided"] + [("lonely", r, s) for r, s in SWITCH_LONELY]


def switch_calls(miss):
    inp = Inp(SWITCH["K"], SWITCH["N"], "scattered", miss)
    fam = "switch " + (miss if isinstance(miss, str) else "lonely")
    return [Call(fam, inp, "count", SWITCH["w"], SWITCH["w"], SWITCH[k], THR) for k in ("atomic", "plain")]


def thin_calls():
    inp = Inp(THIN["K"], THIN["N"], "scattered", "random")
    return [Call("thin", inp, "count", THIN["w"], THIN["wmax"], THIN[k], THR) for k in ("atomic", "plain")]


def split3_calls():
    inp = Inp(SPLIT3["K"], SPLIT3["N"], "scattered", "random")
    return [Call("split3", inp, "count", SPLIT3["w"], SPLIT3["wmax"], SPLIT3["band"], THR)]


def missing_patterns(K, N):
    return ["none", "random", "sided"] + [("lonely", r, s) for r in lonely_rows(K) for s in lonely_samples(N)]


def missing_calls(K, N, miss):
    inp = Inp(K, N, "scattered", miss)
    fam = "missing " + (miss if isinstance(miss, str) else "lonely")
    return [Call(fam, inp, "count", 33, 36, (0, K), THR), Call(fam, inp, "count", 65, 65, (0, K), THR)]


THRESHOLD_INP = Inp(130, 385, "scattered", "none")
SUBSET_CALL = Call("subsets", Inp(130, 385, "scattered", "random"), "count", 65, 68, (0, 130), THR)


def threshold_calls():
    return [Call("threshold", THRESHOLD_INP, "count", 65, 65, (0, 130), t) for t in ("one", "below one")]


def every_call():
    """every device call of this module that returns numbers"""
    out = []
    for N in (129, 385):
        for inp in _edge_inputs(N):
            out += edge_calls(inp)
    out += band_calls()
    for N in SAMPLE_EDGES:
        out += sample_calls(N)
    for miss in SWITCH_MISS:
        out += switch_calls(miss)
    out += thin_calls() + split3_calls()
    for K, N in MISSING_SHAPES:
        for miss in missing_patterns(K, N):
            out += missing_calls(K, N, miss)
    return out + threshold_calls() + [SUBSET_CALL]


# ---------------------------------------------------------------------------------------------------------------------------------
# models of the calls (cached; the large ones one at a time, and the lonely and sided ones as patches of ``none``)
# ---------------------------------------------------------------------------------------------------------------------------------
_MODELS, _BIG = {}, {}


def _fresh_model(call, band=None):
    G, keep = make_input(call.inp)
    r0, r1 = band or call.band
    return ld_model(G, keep, win_end_of(call)[r0:r1], call.wmax, r0, r1)


def _big_model(call):
    """the model of the widest band of a large handle from row 0.  A pattern that changes a few rows of ``none`` is the model of ``none``
    with the rows recomputed whose windows can hold a changed row (the model is a function of rows i .. win_end[i] - 1 alone)."""
    top = max(c.band[1] for c in every_call() if c.inp == call.inp and c.wmax == call.wmax)
    key = (call.inp, call.win, call.w, call.wmax, top)
    if key in _BIG:
        return _BIG[key]
    base_inp = call.inp._replace(miss="none")
    whole = call._replace(band=(0, top))
    if call.inp.miss in ("none", "random"):
        mdl = _fresh_model(whole)
    else:
        base = _big_model(call._replace(inp=base_inp))
        (G0, keep), (G1, _) = make_input(base_inp), make_input(call.inp)
        kb = keep.astype(bool)
        changed = np.flatnonzero((G0[kb] != G1[kb]).any(axis=1))
        assert 0 < changed.size <= 4
        r2, cnt = base.r2.copy(), base.counts.copy()
        for r in changed:
            lo, hi = max(0, int(r) - call.wmax), min(int(r) + 1, top)
            if lo < hi:
                part = _fresh_model(whole, band=(lo, hi))
                r2[lo:hi], cnt[lo:hi] = part.r2, part.counts
        mdl = Model(r2, cnt, base.inwin)
    for k in [k for k in _BIG if k[0].miss != "none" or (k[0].K, k[0].N) != (call.inp.K, call.inp.N)]:
        del _BIG[k]                                                     # (keep the ``none`` base of this shape and the newest)
    _BIG[key] = mdl
    return mdl


def model_of(call):
    r0, r1 = call.band
    if call.inp.K > 4096:
        assert r0 == 0
        big = _big_model(call)
        return Model(big.r2[:r1], big.counts[:r1], big.inwin[:r1])
    key = (call.inp, call.win, call.w, call.wmax, call.band)
    if key not in _MODELS:
        _MODELS[key] = _fresh_model(call)
    return _MODELS[key]


def thr_of(call):
    """the threshold of the call; "one" and "below one" are r2 values the model attains"""
    if not isinstance(call.thr, str):
        return call.thr
    r2 = model_of(call._replace(thr=THR)).r2
    assert (r2 == 1.0).any()
    if call.thr == "one":
        return 1.0
    below = r2[np.isfinite(r2) & (r2 < 1.0) & (r2 > 0.0)]
    return float(below.max())


def products_of(mdl):
    """the largest of n sxy, sx sy, n sxx, sx^2, n syy, sy^2 over the band (Python int)"""
    big = 0
    for a in range(0, mdl.counts.shape[0], 1024):
        c = mdl.counts[a:a + 1024].astype(np.int64)
        n, sx, sy, sxx, syy, sxy = (c[..., s] for s in range(6))
        big = max([big] + [int(np.abs(x).max(initial=0)) for x in (n * sxy, sx * sy, n * sxx, sx * sx, n * syy, sy * sy)])
    return big


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------------------------------------------------------------
def test_model_equals_python_ints():
    for inp, w, wmax, band in ((Inp(14, 9, "scattered", "random"), 5, 8, (0, 14)), (Inp(40, 21, "scattered", "sided"), 33, 33, (3, 38))):
        G, keep = make_input(inp)
        G = G.copy()
        kr = np.flatnonzero(keep)
        G[kr[[0, 5, inp.K - 1]], [1, 4, inp.N - 1]] = MISSING            # (so few samples at 2 % would hold few missing calls)
        call = Call("x", inp, "ragged", w, wmax, band, THR)
        we = win_end_of(call)[band[0]:band[1]]
        mdl = ld_model(G, keep, we, wmax, *band)
        assert mdl.counts.any() and np.isnan(mdl.r2).any() and (mdl.counts[..., 3] != mdl.counts[..., 1]).any()
        want = ld_model_python_ints(G, keep, we, wmax, *band)
        assert mdl.counts.tolist() == want
        for t in range(band[1] - band[0]):                               # r2 from the Python integers, in Python floats
            for d in range(wmax):
                n, sx, sy, sxx, syy, sxy = want[t][d]
                cov, vx, vy = n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy
                inw = band[0] + t + 1 + d < we[t]
                r = 0.0 if not inw else (float("nan") if vx <= 0 or vy <= 0 else (float(cov) * float(cov)) / (float(vx) * float(vy)))
                assert (math.isnan(r) and math.isnan(mdl.r2[t, d])) or r == mdl.r2[t, d], (t, d)
    # against the older numpy reference (f32 products): a shared mistake of the two would have to survive both restatements
    from test_gpu_ld import ref_ld
    call = Call("x", Inp(129, 385, "scattered", "random"), "ragged", 70, 73, (5, 120), THR)
    G, keep = make_input(call.inp)
    we = win_end_of(call)[5:120]
    mdl = ld_model(G, keep, we, 73, 5, 120)
    r2, cnt = ref_ld(G, keep, we, 73, 5, 120)
    assert np.array_equal(mdl.counts, cnt) and np.array_equal(mdl.r2, r2, equal_nan=True)
    words = above_words(mdl.r2, mdl.inwin, 0.2)
    assert words.shape == (115, 2) and words.dtype == np.uint64
    bits = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :73].astype(bool)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(bits, r2 > 0.2) and bits.any()


def test_every_case_is_in_the_exact_regime():
    biggest, label = 0, None
    calls = every_call()
    widest = {}                                                         # (a large handle: once, over its widest band, which holds the others)
    for call in calls:
        if call.inp.K > 4096:
            key = (call.inp, call.wmax)
            if key not in widest:
                widest[key] = products_of(_big_model(call))
            big = widest[key]
        else:
            big = products_of(model_of(call))
        assert big < 2 ** 53, (call, math.log2(big))
        if big > biggest:
            biggest, label = big, call
    print(f"{len(calls)} calls, the largest product = 2^{math.log2(biggest):.2f} ({label.family}, K = {label.inp.K}, N = {label.inp.N})")


def _triples():
    return sorted({(c.band[1] - c.band[0], band_weff(c), c.inp.N) for c in every_call()})


def test_plan_mirror_equals_the_header(tmp_path):
    exe = str(tmp_path / "ld_plan_audit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "genomic_pca_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ld_plan_audit.cpp"), "-o", exe])
    rng = np.random.default_rng(23)
    triples = _triples() + [(int(1 + rng.integers(0, 3_000_000)), int(rng.integers(0, 5000)), int(1 + rng.integers(0, 200_000))) for _ in range(200)]
    triples += [(7232, 1000, 385), (7233, 1000, 385), (3648, 1000, 600), (500_000, 200, 50_000)]
    args = [str(v) for t in triples for v in t]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(triples)
    for t, line in zip(triples, lines):
        p = ld_plan(*t)
        assert line == f"{t[0]} {t[1]} {t[2]}: {p.workgroups} {p.chunks} {p.stages} {p.per} {p.splits} {p.kind}", (t, line)
    assert ld_plan(500_000, 200, 50_000) == Plan(23439, 3, 391, 391, 1, "plain")       # the production shape of the issue
    print(f"{len(triples)} plans equal the header's")


def regime_gaps(calls):
    """the names of the plan regimes the calls do not contain"""
    launched = [(c, plan_of(c), band_weff(c)) for c in calls if band_weff(c) > 0 and c.band[1] > c.band[0]]
    have = set()
    for c, p, weff in launched:
        stages = min(p.per, 3)
        have.add((p.kind, stages))
        if p.kind == "atomic" and p.stages % p.per:
            have.add("short last split")
        have.add(("chunks", min(p.chunks, 3)))
        have.add(("weff", weff))
        r0, r1 = c.band
        have.add(("row0 % 64", r0 % 64))
        if r1 < c.inp.K and int(win_end_of(c)[r0:r1].max()) > r1:
            have.add("windows past row1")
    for c in calls:
        have |= {("K", c.inp.K), ("N % 16", c.inp.N % 16), ("N % 128", c.inp.N % 128), ("wmax", c.wmax)}
    want = [(kind, s) for kind in ("plain", "atomic") for s in (1, 2, 3)] + ["short last split", "windows past row1"]
    want += [("chunks", n) for n in (1, 2, 3)] + [("weff", w) for w in (32, 33, 64, 65, 192, 193)] + [("K", K) for K in K_EDGES]
    want += [("row0 % 64", r) for r in (0, 1, 63)] + [("N % 16", r) for r in (0, 1, 15)] + [("N % 128", r) for r in (0, 1, 127)]
    want += [("wmax", w) for w in (63, 64, 65, 256, 257)]
    return [w for w in want if w not in have]


def test_every_plan_regime_is_covered():
    calls = every_call()
    assert regime_gaps(calls) == []
    a, p = (plan_of(c) for c in switch_calls("none"))
    assert a == Plan(1017, 9, 4, 2, 2, "atomic") and p == Plan(1026, 9, 4, 4, 1, "plain")
    a, p = (plan_of(c) for c in thin_calls())
    assert a == Plan(1022, 2, 2, 1, 2, "atomic") and p == Plan(1024, 2, 2, 2, 1, "plain")
    assert plan_of(split3_calls()[0]) == Plan(514, 2, 5, 3, 2, "atomic")
    # the list has no slack where it matters: without the switch pair, or without either side of 64 | 65, a regime is missing
    assert ("plain", 3) in regime_gaps([c for c in calls if not c.family.startswith("switch")])
    assert ("atomic", 2) in regime_gaps([c for c in calls if not c.family.startswith("switch")])
    for w in (64, 65):
        assert ("weff", w) in regime_gaps([c for c in calls if band_weff(c) != w])
    kinds = {}
    for c in calls:
        if band_weff(c) > 0:
            p = plan_of(c)
            kinds[(p.kind, min(p.per, 3))] = kinds.get((p.kind, min(p.per, 3)), 0) + 1
    print(f"{len(calls)} calls; launches by (stores, stages per split, 3 = three or more): {sorted(kinds.items())}")


PLANE_MUTANTS = ("last stage dropped", "last split dropped", "column tail read as zero", "sides swapped", "g' for g'^2 against a missing call",
                 "saw_missing from the first stage only")
MUTANTS = PLANE_MUTANTS + ("pad samples counted in n", "j <= win_end", "last slot of the widest window dropped", ">= for the threshold",
                           "counts left outside the window")
_NO_MISSING = {"switch none", "missing none", "threshold"}              # no missing call anywhere: g'm = mg' = qm = mq = 0
_FULL_WINDOWS = {"switch none", "switch random", "switch lonely", "switch sided"}   # wmax = w and every window is full: no slot outside
_BELOW_K = _FULL_WINDOWS | {"thin", "split3"}                           # no window reaches the last multiple of 32 below K
# plain stores, more than one stage and a pair of rows whose missing calls all lie after the first: everything else is atomic, or one
# stage, or without missing calls, or (``sided``: a quarter of a row) has them in every stage
_LATE_MISSING = ("switch random", "switch lonely", "thin")
CANNOT_TOUCH = {
    "sides swapped": _NO_MISSING, "g' for g'^2 against a missing call": _NO_MISSING,
    "j <= win_end": _FULL_WINDOWS,                                      # slot win_end - i - 1 is past wmax in every row
    "column tail read as zero": _BELOW_K,
    ">= for the threshold": None,                                       # every family but "threshold": THR is not attained
    "counts left outside the window": _FULL_WINDOWS | {"threshold"},    # ("threshold": wmax = w, the only slots outside have j >= K)
    "saw_missing from the first stage only": "not " + " ".join(_LATE_MISSING),
}


def _moved(call, mut):
    """whether the mutant moves a compared bit of the call (large calls: of its first or its last 128 rows)"""
    r0, r1 = call.band
    mid = min(max(call.inp.K // 4 - 64, r0), r1 - 128)                  # (the rows of ``sided`` are K // 4 .. K // 4 + 4)
    bands = [(r0, r1)] if r1 - r0 <= 512 else [(r0, r0 + 128), (mid, mid + 128), (r1 - 128, r1)]
    G, keep = make_input(call.inp)
    thr = thr_of(call)
    plan, weff = plan_of(call), band_weff(call)
    for a, b in bands:
        we = win_end_of(call)[a:b]
        base = ld_model(G, keep, we, call.wmax, a, b) if (a, b) != call.band else model_of(call)
        if mut == ">= for the threshold":
            if not np.array_equal(above_words(base.r2, base.inwin, thr), above_words(base.r2, base.inwin, thr, ge=True)):
                return True
            continue
        m = ld_model(G, keep, we, call.wmax, a, b, mut=mut, plan=plan, weff=weff)
        if not (np.array_equal(m.r2, base.r2, equal_nan=True) and np.array_equal(m.counts, base.counts)
                and np.array_equal(above_words(m.r2, m.inwin, thr), above_words(base.r2, base.inwin, thr))):
            return True
    return False


def test_teeth():
    """every mutant moves a compared bit in at least one call of every family it can touch, and none in a family it cannot"""
    families = {}
    for c in every_call():
        if band_weff(c) > 0:
            families.setdefault(c.family, []).append(c)
    assert set(families) >= {"edges", "bands", "samples", "thin", "split3", "threshold", "subsets"} | _FULL_WINDOWS | {"missing " + k for k in ("none", "random", "lonely", "sided")}
    for mut in MUTANTS:
        cannot = CANNOT_TOUCH.get(mut, set())
        if cannot is None:
            cannot = set(families) - {"threshold"}
        elif isinstance(cannot, str):
            cannot = set(families) - set(_LATE_MISSING)
        bitten = 0
        for fam, calls in families.items():
            if fam == "edges":                                          # (one handle per K of one sample count is plenty)
                calls = [c for c in calls if c.inp.N == 385]
            if fam in cannot:
                assert not any(_moved(c, mut) for c in calls), (mut, fam)
            else:
                assert any(_moved(c, mut) for c in calls), (mut, fam)
                bitten += 1
        print(f"{mut}: {bitten} families bitten, {len(cannot)} out of reach and untouched")
    # the lonely call: saw_missing under plain stores needs it in a stage after the first -- the planes of the last three stages hold it
    late = [c for c in switch_calls(("lonely", 63, 128)) if plan_of(c).kind == "plain"]
    assert late and all(_moved(c, "g' for g'^2 against a missing call") or _moved(c, "sides swapped") for c in late)


# ---------------------------------------------------------------------------------------------------------------------------------
# device tests
# ---------------------------------------------------------------------------------------------------------------------------------
def open_handle(e, inp):
    G, keep = make_input(inp)
    M = G.shape[0]
    e.upload_genotypes_i8(G)
    e.snp_stats(gpca.QcConfig.none())
    e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), keep)
    assert np.array_equal(e.pca_snp_rows(), np.flatnonzero(keep))


def run_call(e, call):
    """the device's r2, counts and above of one call (bands of more than 2 M slots in two calls, to bound the buffers)"""
    r0, r1 = call.band
    we = win_end_of(call)[r0:r1]
    thr = thr_of(call)
    if (r1 - r0) * call.wmax <= 2_000_000:
        return e.ld_window(we, wmax=call.wmax, rows=call.band, threshold=thr, counts=True)
    out = e.ld_window(we, wmax=call.wmax, rows=call.band, threshold=thr, counts=True, r2=False)
    out["r2"] = e.ld_window(we, wmax=call.wmax, rows=call.band)["r2"]
    return out


def check_call(e, call, label):
    out = run_call(e, call)
    mdl = model_of(call)
    rows = call.band[1] - call.band[0]
    assert out["r2"].shape == (rows, call.wmax) and out["counts"].shape == (rows, call.wmax, 6) and out["above"].shape == (rows, (call.wmax + 63) // 64)
    bad = np.argwhere(out["counts"] != mdl.counts)
    assert bad.size == 0, (label, call, f"{len(bad)} counts differ, first at (t, d, s) = {bad[0].tolist()}: {out['counts'][tuple(bad[0])]} for {mdl.counts[tuple(bad[0])]}")
    assert np.array_equal(out["r2"], mdl.r2, equal_nan=True), (label, call, "r2")
    assert np.array_equal(out["above"], above_words(mdl.r2, mdl.inwin, thr_of(call))), (label, call, "above")
    RECORD["calls"] += 1; RECORD["comparisons"] += 3
    return out


def _handle_cases(store, inp, calls):
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        open_handle(e, inp)
        for c in calls:
            check_call(e, c, store)
    print(f"{store} K = {inp.K} N = {inp.N}: {len(calls)} calls equal the model; so far {RECORD['calls']} calls, {RECORD['comparisons']} comparisons")


@pytest.mark.gpu
@pytest.mark.parametrize("inp", _edge_inputs(129) + _edge_inputs(385), ids=lambda i: f"K{i.K}-N{i.N}-{i.keep.replace(' ', '_')}")
@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_kept_row_and_window_edges_equal_the_model(store, inp):
    _handle_cases(store, inp, edge_calls(inp))


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_bands_equal_the_model(store):
    calls = band_calls()
    _handle_cases(store, calls[0].inp, calls)


@pytest.mark.gpu
@pytest.mark.parametrize("N", SAMPLE_EDGES)
@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_sample_edges_equal_the_model(store, N):
    calls = sample_calls(N)
    _handle_cases(store, calls[0].inp, calls)


@pytest.mark.gpu
@pytest.mark.parametrize("miss", SWITCH_MISS, ids=lambda m: m if isinstance(m, str) else f"lonely-{m[1]}-{m[2]}")
@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_plain_and_atomic_bands_at_the_switch_equal_the_model(store, miss):
    """1 017 workgroups (atomic, 2 x 2 stages) and 1 026 (plain stores, 4 stages) on one handle: both equal the model, and the rows they
    share are bit-identical"""
    atomic, plain = switch_calls(miss)
    assert plan_of(atomic).kind == "atomic" and plan_of(plain).kind == "plain" and plan_of(plain).per >= 3
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        open_handle(e, atomic.inp)
        a = check_call(e, atomic, store)
        p = check_call(e, plain, store)
    n = atomic.band[1]
    assert np.array_equal(a["counts"], p["counts"][:n]) and np.array_equal(a["r2"], p["r2"][:n], equal_nan=True) and np.array_equal(a["above"], p["above"][:n])
    RECORD["comparisons"] += 3


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_plain_stores_with_two_stages_equal_the_model(store):
    atomic, plain = thin_calls()
    assert plan_of(plain) == Plan(1024, 2, 2, 2, 1, "plain") and plan_of(atomic).kind == "atomic"
    _handle_cases(store, plain.inp, [atomic, plain])


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_atomic_splits_of_three_and_two_stages_equal_the_model(store):
    (call,) = split3_calls()
    assert plan_of(call) == Plan(514, 2, 5, 3, 2, "atomic")
    _handle_cases(store, call.inp, [call])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["none", "random", "sided", "lonely"])
@pytest.mark.parametrize("K,N", MISSING_SHAPES)
@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_missing_patterns_equal_the_model(store, K, N, kind):
    for miss in missing_patterns(K, N):
        if (miss if isinstance(miss, str) else miss[0]) == kind:
            calls = missing_calls(K, N, miss)
            _handle_cases(store, calls[0].inp, calls)


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_threshold_is_strictly_greater(store):
    calls = threshold_calls()
    thrs = [thr_of(c) for c in calls]
    mdl = model_of(calls[0])
    assert thrs[0] == 1.0 and 0.0 < thrs[1] < 1.0
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        open_handle(e, THRESHOLD_INP)
        for c, t in zip(calls, thrs):
            out = check_call(e, c, store)
            bits = np.unpackbits(out["above"].view(np.uint8), axis=1, bitorder="little")[:, :c.wmax].astype(bool)
            at = mdl.r2 == t
            assert at.any() and not bits[at].any()                       # attained, and not above itself
            if t < 1.0:
                assert bits[mdl.r2 == 1.0].all()


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_output_subsets_equal_the_full_call(store):
    """the seven non-empty subsets of {r2, counts, above} through the C ABI (the wrapper cannot ask for counts alone)"""
    call = SUBSET_CALL
    lib = _lib.load()
    r0, r1 = call.band
    rows, wmax = r1 - r0, call.wmax
    we = np.ascontiguousarray(win_end_of(call)[r0:r1], np.int64)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        open_handle(e, call.inp)
        full = check_call(e, call, store)
        for mask in range(1, 8):
            bufs = {"r2": np.full((rows, wmax), 7.0), "counts": np.full((rows, wmax, 6), 7, np.int32), "above": np.full((rows, (wmax + 63) // 64), 7, np.uint64)}
            ptr = lambda k, bit: bufs[k].ctypes.data if mask & bit else None
            rc = lib.gpca_ld_window(e._h, r0, r1, we.ctypes.data, wmax, call.thr, ptr("r2", 1), ptr("counts", 2), ptr("above", 4))
            assert rc == _lib.GPCA_OK, (mask, lib.gpca_last_error(e._h).decode())
            for k, bit in (("r2", 1), ("counts", 2), ("above", 4)):
                if mask & bit:
                    assert np.array_equal(bufs[k], full[k], equal_nan=k == "r2"), (mask, k)
                    RECORD["comparisons"] += 1
                else:
                    assert (bufs[k] == 7).all(), (mask, k)               # an output that was not asked for is not written


@pytest.mark.gpu
def test_every_invalid_byte_is_refused_and_named():
    """int8 storage: each of the 252 byte values outside {0, 1, 2, 0x81} in one kept row of a 70 x 37 matrix, 252 calls on one handle"""
    M, N, w = 70, 37, 20
    rng = np.random.default_rng(29)
    G0 = rng.integers(0, 3, size=(M, N)).astype(np.int8)
    G0[rng.random((M, N)) < 0.03] = MISSING
    keep = np.ones(M, np.uint8); keep[[4, 40]] = 0
    kr = np.flatnonzero(keep)
    K = kr.size
    we = np.minimum(np.arange(K, dtype=np.int64) + 1 + w, K)
    lib = _lib.load()
    r2 = np.zeros((K, w))
    ones = np.ones(M, np.float32)
    bad_bytes = [b for b in range(256) if b not in (0, 1, 2, 0x81)]
    assert len(bad_bytes) == 252

    def call(e, r0=0, r1=K):
        win = np.ascontiguousarray(we[r0:r1])
        return lib.gpca_ld_window(e._h, r0, r1, win.ctypes.data, w, 0.2, r2.ctypes.data, None, None)

    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        for n, b in enumerate(bad_bytes):
            G = G0.copy()
            row = int(kr[(7 * n) % K])
            G[row, (0, 15, 16, 36)[n % 4]] = np.uint8(b).astype(np.int8)
            e.upload_genotypes_i8(G)
            e.set_standardization(ones, ones, keep)
            assert call(e) == _lib.GPCA_ERR_INVALID_GENOTYPE, hex(b)
            assert f"row {row} " in lib.gpca_last_error(e._h).decode(), (hex(b), row, lib.gpca_last_error(e._h).decode())
        # two bad rows in different workgroups of k_ld_vec (four rows each): the smaller original row is named
        G = G0.copy()
        G[kr[50], 16] = 3; G[kr[9], 36] = -1
        e.upload_genotypes_i8(G)
        e.set_standardization(ones, ones, keep)
        assert call(e) == _lib.GPCA_ERR_INVALID_GENOTYPE and f"row {int(kr[9])} " in lib.gpca_last_error(e._h).decode()
        assert call(e, 10, K) == _lib.GPCA_ERR_INVALID_GENOTYPE and f"row {int(kr[50])} " in lib.gpca_last_error(e._h).decode()
        assert call(e, 51, K) == _lib.GPCA_OK                            # a band whose rows and windows do not reach either row
        assert call(e, 10, 50 - w) == _lib.GPCA_OK                       # rows 10 .. 29 read kept rows 10 .. 49
        assert call(e, 10, 50 - w + 1) == _lib.GPCA_ERR_INVALID_GENOTYPE # ... and one more row reaches kept row 50
        # a bad byte in a row that is not kept
        G = G0.copy()
        G[4, 0] = 3; G[40, 36] = -128
        e.upload_genotypes_i8(G)
        e.set_standardization(ones, ones, keep)
        assert call(e) == _lib.GPCA_OK
        want = ld_model(G0, keep, we, w)
        assert np.array_equal(r2, want.r2, equal_nan=True)
