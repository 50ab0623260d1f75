"""gpca_grm held to its exact integer model (grm.hip, gpca_grm.cpp) at every tile edge.

THE MODEL.  ``grm_model(G, mu, sigma, keep, scaling)`` restates the call from its inputs alone.  r and b are k_set_scale's (f32 1 / sigma,
f32 -mu r, 0 on a row that is not kept or has |sigma| < 1e-9; centred: r = 1, b = -mu in f64).  w = r^2, 2w, c = -r b and e = b^2 are exact
f64 products of f32 values; vmax = max(2w, c, e) over the kept rows; S is the smallest power of two with vmax / S <= 128^6 - 1; every table
is q = llround(x / S) -- half away from zero, 2w rounded on its own.  Then, all in exact integers,
    R_ab = sum_i g'_a q_i(g'_b w) + g'_a m_b q_i(c) + m_a g'_b q_i(c) + m_a m_b q_i(e)      (b <= a; q(g' w) = q(w) for g' = 1, q(2w) for g' = 2)
    u_a = sum_i q_i(c) g'_a,   v_a = sum_i q_i(e) m_a,   beta = sum_i q_i(e)
    I_ab = ((((R_ab - u_a) - u_b) + beta) - v_a) - v_b                                      (the order of k_grm_finish)
    GRM_ab = float(I_ab) S / K,   NPAIRS_ab = K - cnt_a - cnt_b + sum_i m_a m_b
over the K kept rows (a kept row with r = b = 0 has zero tables and still counts in K and NPAIRS).  The sums go through f64 matmuls of
limbs of q (``int_gram``: the limb width is the widest with every partial sum below 2^53, 21 bits at these shapes, 14 on request),
recombined in int64; test_model_equals_python_ints checks that against plain Python integers.  ``big`` is the largest magnitude of any
integer the device forms (R -- whose terms are all >= 0, so its partial sums are covered --, u, v, beta and every intermediate of the
finish chain); ``mag`` is (R + u_a + u_b + beta + v_a + v_b) S / K per element.

THE TWO BARS (``check_device``).
* big < 2^53: every i32 -> f64 conversion, every fma(s, 128, acc[d]) of the fold, every running-sum addition, every int64 -> f64
  conversion of u and v, every step of the finish and the product by S is exact, whatever the flush groups and panels are; the division by
  K rounds once, as the model's does.  The device output is then a function of the inputs alone and is compared with np.array_equal on the
  lower triangle.  NPAIRS is compared exactly in either regime.
* otherwise every f64 operation rounds once, relative error at most u = 2^-53 of a quantity bounded by mag (in units of S / K).  Counted
  from the code, with P the number of flush groups over all panels: the 5 fma of a group's fold act on that group's partial and cost 5u R
  in total; one addition per group to the running sum, P u R; per group one int64 -> f64 conversion of the partial of u (of v) and one
  addition in k_grm_vec_fold, (P + 1) u u_a each; one rounding of beta; 5 roundings in the finish, each of a value bounded by the sum of
  the magnitudes; one in the division.  To first order that is (P + 11) u mag; the bar asserted is the issue's
      |device - model| <= (2 P + 12) 2^-53 mag_ab                                             per element
  which covers it with the second-order terms to spare.  On W ranks each rank rounds over its own rows and the exchange adds W - 1 sums:
  (2 P + 12 W + W - 1) u mag with P summed over the ranks.

THE MODEL AGAINST THE F64 REFERENCE ``ref_grm`` (CPU).  Each table value is off by at most S / 2, and that enters the product, u, v and
beta, so with n_ab = sum_i [g'_a([g'_b > 0] + m_b) + m_a(g'_b + m_b)] + sum g'_a + sum g'_b + K + sum m_a + sum m_b over the kept rows
    |model_ab - truth_ab| <= (S / 2K) n_ab + u |model_ab|                                     (the model's one division)
and ref_grm itself is off from the truth by at most (K + 4) u sum_i |Z_ia| |Z_ib| / K: one rounding in Z = r g + b (r g is exact), one per
product, K - 1 additions in any order and one division.  test_model_within_quantisation_bar asserts the sum of the two per element.

INPUTS (seeded, ``make_input``).  Where the shape allows (M >= 12; the one shape below is M = 1) every input has a row that is not kept,
holds the invalid call 3 and has a NaN sigma (row 5), a kept row with sigma = 1e-10 (row 7: r = b = 0) and a kept row with mu = 0 (row 9).
Under 2-bit storage the invalid call is stored as a missing one; the row is not kept, so the model does not move.  Families: ``centred``
(any f32 mu, centred scaling: nothing of the scale is computed on the device), ``pow2`` (sigma in {1, 1/2, .., 1/32}: r and b are exact
whatever the device's division does, vmax = 2^11 and S = 2^-30 exactly on the edge of the search), ``generic`` (sigma = sqrt(2p(1 - p)), p
in [0.05, 0.5]: all six planes, q(2w) != 2 q(w) on about half the rows), ``spread`` (generic with one kept row at p = 1e-4: S = 2^-28,
the common rows lose their low planes), ``tie`` (centred, means chosen so that c / S lies exactly on .5 in two rows: llround against
rint).  Missing patterns: none, 2 % at random, and ``lonely`` -- one missing call in the whole matrix, at row in {0, 31, 32, M - 1} x sample
in {0, 31, 32, 63, 64, N - 1}, aimed at the wave ballot and the a-side / b-side terms.  Shapes: EDGE_M at 65 samples and EDGE_N at 33 rows
with the keeps of edge_keeps (generic, both scalings), the four families at 4097 x 129, lonely at 33 x 129 and 4097 x 129, panels of 8192,
3072 and 1000 (rounded up to 1024 by gpca_stream_open) rows at 7169 rows, two ranks through the allreduce hook with the rare row on rank 1,
and the band (65, 129).  test_every_case_is_in_the_exact_regime asserts big < 2^53 for every one of them on the CPU.

TEETH (CPU).  ``MUTANTS`` are changes of the model; test_teeth asserts that each moves at least one bit of the lower triangle (of NPAIRS
for the count mutant) in at least one case of every family it can touch, and that the ones that cannot touch a family leave it alone:
the side swap and 2 q(w) for q(2w) cannot touch ``centred`` and ``pow2`` (w is a power of two there, so q(2w) = 2 q(w) and the product is
symmetric); a dropped plane touches a family where some kept row has a nonzero digit in it (and, for c and e, a missing call) -- computed
from the tables, and the planes that are zero throughout a family are listed in ZERO_PLANES and asserted to be exactly those; v without
the keep mask touches ``centred`` only (under the standardized scaling a row that is not kept has b = 0).

RECORDS (not thresholds; each test prints its own with -s).  On one MI355X the 168 device cases of this module take 8 s and make 482
comparisons with the model: all 482 in the exact regime and bit-equal, none under the rounding bar -- ``generic`` included, so the
handle's r is the correctly rounded f32 reciprocal on every row -- and panels of 3 072 and 1 024 rows give the bits of the resident call.
The largest big is 2^52.58 (8193 x 65, centred).  The 6 CPU tests take 25 s (the teeth most of it).  The model sits within the
quantisation bar against ref_grm by a largest fraction of 0.999 (33 x 257 with one kept row: with K = 1 the scale follows the row, x / S
keeps six fraction bits and one table value lies exactly on .5, so S / 2 is attained; at most 0.05 with 4 096 kept rows and more).
The rounding bar is reached by one case of tests/test_gpu_grm.py only (20 000 x 700 centred, big = 2^53.64): largest fraction 0.034,
resident and streamed.
"""
import math
from collections import namedtuple

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from _edges import EDGE_M, EDGE_N, edge_keeps

QMAX = 128 ** 6 - 1
DIGITS = 6
FLUSH = 4096
U64 = 2.0 ** -53
MISSING = -127
STORES = {"int8": _lib.STORE_INT8, "2bit": _lib.STORE_2BIT}
TABLES = ("w", "w2", "c", "e")
RECORD = {"big": 0, "quant": 0.0, "exact": 0, "rounded": 0}

Model = namedtuple("Model", "grm npairs big mag S K I q")


# ---------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------
def scale_rb(mu, sigma, keep, scaling):
    """r, b in f64 as gpca_grm's host scan reads them: k_set_scale's f32 values (standardized) or 1, -mu (centred); 0 where not kept"""
    mu = np.asarray(mu, np.float32); sigma = np.asarray(sigma, np.float32); keep = np.asarray(keep).astype(bool)
    if scaling == "centred":
        return np.where(keep, 1.0, 0.0), np.where(keep, -mu.astype(np.float64), 0.0)
    with np.errstate(all="ignore"):
        ok = keep & ~(np.abs(sigma) < np.float32(1e-9))
        r = np.where(ok, np.float32(1.0) / np.where(ok, sigma, np.float32(1)), np.float32(0)).astype(np.float32)
        b = np.where(ok, (-mu * r).astype(np.float32), np.float32(0)).astype(np.float32)
    return r.astype(np.float64), b.astype(np.float64)


def round_half_away(x):
    """llround of x >= 0 (x - trunc(x) is exact)"""
    t = np.trunc(x)
    return (t + (x - t >= 0.5)).astype(np.int64)


def round_half_even(x):
    return np.rint(x).astype(np.int64)


def pick_scale(vmax):
    """the smallest power of two S with vmax / S <= 128^6 - 1 (1 for vmax = 0)"""
    if vmax <= 0.0:
        return 1.0
    S = 2.0 ** math.frexp(vmax / QMAX)[1]
    while vmax / (S * 0.5) <= QMAX:
        S *= 0.5
    while vmax / S > QMAX:
        S *= 2.0
    return S


def quantise(mu, sigma, keep, scaling, rounding=round_half_away, s_steps=0, vmax_extra=0.0, every_row=False):
    """S and the four int64 tables [M] (0 on rows that are not kept).  every_row: tables of the rows that are not kept too (a mutant)"""
    keepb = np.asarray(keep).astype(bool)
    r, b = scale_rb(mu, sigma, keepb, scaling)
    if every_row and scaling == "centred":
        r = np.ones(len(keepb)); b = -np.asarray(mu, np.float32).astype(np.float64)
    w, c, e = r * r, -r * b, b * b
    kept = [x[keepb] for x in (w, c, e)]
    assert all(np.all(np.isfinite(x)) for x in kept) and np.all(kept[1] >= 0), "gpca_grm refuses this input"
    vmax = max([vmax_extra] + [float(np.max(x)) if x.size else 0.0 for x in (2.0 * kept[0], kept[1], kept[2])])
    S = pick_scale(vmax) * 2.0 ** s_steps
    sel = np.ones_like(keepb) if every_row else keepb
    q = {k: np.where(sel, rounding(np.where(sel, x, 0.0) / S), 0).astype(np.int64) for k, x in (("w", w), ("w2", 2.0 * w), ("c", c), ("e", e))}
    return S, q


def int_gram(pairs, N, limb_bits=None):
    """exact int64 sum over (L, X) of L^T X: L [rows][N] in {0, 1, 2}, X [rows][N] int64 >= 0.  Limbs of X go through f64 matmuls; the limb
    width keeps every partial sum below 2^53, so each matmul is exact in any summation order."""
    L = np.concatenate([p[0] for p in pairs]); X = np.concatenate([p[1] for p in pairs])
    live = L.any(axis=1) & X.any(axis=1)
    L, X = L[live], X[live]
    out = np.zeros((N, N), np.int64)
    if not L.shape[0]:
        return out
    assert L.min() >= 0 and L.max() <= 2 and X.min() >= 0
    bits = limb_bits or min(21, 51 - max(int(L.shape[0]), 1).bit_length())
    assert 2 * (2 ** bits) * L.shape[0] < 2 ** 53
    Lt = np.ascontiguousarray(L.T.astype(np.float64))
    shift = 0
    while True:
        rest = X >> shift
        if not rest.any():
            return out
        limb = (rest & ((1 << bits) - 1)).astype(np.float64)
        part = Lt @ limb
        assert part.max() < 2.0 ** 53
        out += part.astype(np.int64) << shift
        shift += bits


def block_flags(G, N):
    """[row][sample] -> whether the 32-row block x 32-sample group of the call holds a missing call (what one side of the ballot sees)"""
    M = G.shape[0]
    m = np.zeros((-(-M // 32) * 32, -(-N // 32) * 32), bool)
    m[:M, :N] = G == MISSING
    f = m.reshape(m.shape[0] // 32, 32, m.shape[1] // 32, 32).any(axis=(1, 3))
    return np.repeat(np.repeat(f, 32, axis=0), 32, axis=1)[:M, :N]


def grm_model(G, mu, sigma, keep, scaling, mut=None, limb_bits=None, vmax_extra=0.0):
    """the exact integer model of one gpca_grm call over the whole matrix.  mut: one entry of MUTANTS (teeth only).  vmax_extra: the
    largest table value of the other ranks (a rank's share of a sharded call)"""
    mut = mut or {}
    G = np.asarray(G); M, N = G.shape
    keepb = np.asarray(keep).astype(bool)
    K = int(keepb.sum())
    S, qv = quantise(mu, sigma, keepb, scaling, mut.get("rounding", round_half_away), mut.get("s_steps", 0), vmax_extra)
    qt = {k: v.copy() for k, v in qv.items()}                       # what goes into `tab`; qv's c and e feed u, v and beta
    if "drop_plane" in mut:
        t, d = mut["drop_plane"]
        qt[t] &= ~np.int64(127 << (7 * d))
    if mut.get("w2_is_twice_w"):
        qt["w2"] = 2 * qt["w"]
    X = G[keepb]
    m = X == MISSING
    assert np.all(m | ((X >= 0) & (X <= 2))), "a kept row holds an invalid call"
    ga = np.where(m, 0, X).astype(np.int64); mi = m.astype(np.int64)
    col = lambda k, tab=qt: tab[k][keepb][:, None]
    for_one = col("w2") if mut.get("one_takes_2w") else col("w")
    for_two = col("w") if mut.get("two_takes_w") else col("w2")
    Bw = (ga == 1) * for_one + (ga == 2) * for_two
    ga_b, ga_a = ga, ga                                             # g' as the a-side of g'_a m_b c / as the b-side of m_a g'_b c
    if mut.get("skip_when_only_a_side_missing"):                    # the ballot sees the column side only: m_a g'_b c needs a missing b-group
        ga_a = ga * block_flags(G, N)[keepb]
    if mut.get("skip_when_only_b_side_missing"):                    # ... the row side only: g'_a m_b c needs a missing a-group
        ga_b = ga * block_flags(G, N)[keepb]
    c_in_b = col("e") if mut.get("e_for_c") else col("c")
    pairs = [(ga, Bw), (mi, mi * col("e"))]
    if not mut.get("drop_c_on_b_side"):
        pairs.append((ga_b, mi * c_in_b))
    if not mut.get("drop_c_on_a_side"):
        pairs.append((mi, ga_a * col("c")))
    merged = {}
    for L, Xr in pairs:
        merged[id(L)] = (L, merged[id(L)][1] + Xr) if id(L) in merged else (L, Xr)
    R = int_gram(list(merged.values()), N, limb_bits)
    if mut.get("swap_sides"):
        R = R.T.copy()
    u = (col("w" if mut.get("u_from_w") else "c", qv) * ga).sum(axis=0)
    if mut.get("v_without_keep"):
        _, qa = quantise(mu, sigma, keepb, scaling, every_row=True)
        v = (qa["e"][:, None] * (G == MISSING)).sum(axis=0) if scaling == "centred" else (col("e", qv) * mi).sum(axis=0)
    else:
        v = (col("e", qv) * mi).sum(axis=0)
    qe_kept = qv["e"][keepb]
    beta = int(qe_kept[:-1].sum() if mut.get("beta_short") else qe_kept.sum())
    mn = (G == MISSING).astype(np.float64) if mut.get("npairs_without_keep") else mi.astype(np.float64)
    cnt = mn.sum(axis=0)
    npairs = K - cnt[:, None] - cnt[None, :] + mn.T @ mn
    chain = [R]
    chain.append(chain[-1] - u[:, None]); chain.append(chain[-1] - u[None, :]); chain.append(chain[-1] + beta)
    chain.append(chain[-1] - v[:, None]); chain.append(chain[-1] - v[None, :])
    I = chain[-1]
    il = np.tril_indices(N)
    big = max([beta, int(np.abs(u).max(initial=0)), int(np.abs(v).max(initial=0))] + [int(np.abs(c[il]).max()) for c in chain])
    mag_i = R + u[:, None] + u[None, :] + beta + v[:, None] + v[None, :]
    lower = lambda A: np.where(np.tri(N, dtype=bool), A, A.T)       # the lower triangle, mirrored (GpcaEngine.grm's layout)
    grm = lower(I).astype(np.float64) * S / K
    mag = lower(mag_i).astype(np.float64) * S / K
    return Model(grm, lower(npairs), big, mag, S, K, lower(I), qv)


def grm_model_python_ints(G, mu, sigma, keep, scaling):
    """the same sums with Python integers and plain loops (small shapes only): I [N][N] (lower triangle), npairs, big"""
    G = np.asarray(G); M, N = G.shape
    keepb = np.asarray(keep).astype(bool)
    S, q = quantise(mu, sigma, keepb, scaling)
    rows = [i for i in range(M) if keepb[i]]
    qw, qw2, qc, qe = ([int(x) for x in q[k]] for k in TABLES)
    gp = [[0 if G[i, n] == MISSING else int(G[i, n]) for n in range(N)] for i in range(M)]
    ms = [[int(G[i, n] == MISSING) for n in range(N)] for i in range(M)]
    u = [sum(qc[i] * gp[i][a] for i in rows) for a in range(N)]
    v = [sum(qe[i] * ms[i][a] for i in rows) for a in range(N)]
    beta = sum(qe[i] for i in rows)
    big = max([beta] + u + v)
    I = [[0] * N for _ in range(N)]
    npairs = [[0] * N for _ in range(N)]
    for a in range(N):
        for b in range(a + 1):
            R = 0
            for i in rows:
                gb = gp[i][b]
                R += gp[i][a] * ((qw[i] if gb == 1 else qw2[i] if gb == 2 else 0) + ms[i][b] * qc[i]) + ms[i][a] * (gb * qc[i] + ms[i][b] * qe[i])
            t = [R, R - u[a]]
            t.append(t[-1] - u[b]); t.append(t[-1] + beta); t.append(t[-1] - v[a]); t.append(t[-1] - v[b])
            big = max([big] + [abs(x) for x in t])
            I[a][b] = t[-1]
            npairs[a][b] = sum(1 for i in rows if not ms[i][a] and not ms[i][b])
    return S, I, npairs, big


def flush_groups(M, panel_rows=None):
    """P: the flush groups of 4 096 rows over every panel of the sweep"""
    pr = panel_rows or M
    return sum(-(-min(pr, M - r0) // FLUSH) for r0 in range(0, M, pr))


def check_device(tri, npairs_tri, mdl, P, label, rows=None, ranks=1):
    """the device's packed lower-triangle band against the model: equality where big < 2^53, the rounding bar otherwise.  Returns the regime."""
    N = mdl.grm.shape[0]
    a, b = np.tril_indices(N)
    if rows is not None:
        sel = (a >= rows[0]) & (a < rows[1]); a, b = a[sel], b[sel]
    want, mag = mdl.grm[a, b], mdl.mag[a, b]
    assert tri.shape == want.shape, label
    if npairs_tri is not None:
        assert np.array_equal(npairs_tri, mdl.npairs[a, b].astype(np.float32)), (label, "NPAIRS")
    d = np.abs(tri - want)
    unit = mdl.S / mdl.K
    RECORD["big"] = max(RECORD["big"], mdl.big)
    if mdl.big < 2 ** 53:
        RECORD["exact"] += 1
        bad = np.flatnonzero(tri != want)
        assert bad.size == 0, (label, f"{bad.size} of {tri.size} elements differ from the exact model; the largest by {d.max() / unit:.3g} units of S / K "
                                      f"(mag {mag[np.argmax(d)] / unit:.3g} units), first at (a, b) = ({a[bad[0]]}, {b[bad[0]]})")
        return "exact"
    RECORD["rounded"] += 1
    bar = (2 * P + 12 * ranks + ranks - 1) * U64 * mag
    frac = float(np.max(d / np.maximum(bar, np.finfo(float).tiny)))
    print(f"{label}: big = 2^{math.log2(mdl.big):.2f}, largest fraction of the rounding bar {frac:.3f}")
    assert np.all(d <= bar), (label, frac)
    return "rounded"


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
BAD_ROW, TINY_ROW, ZERO_MU_ROW = 5, 7, 9
FAMILIES = {"centred": "centred", "pow2": "standardized", "generic": "standardized", "spread": "standardized"}
LONELY_ROWS = lambda M: [0, 31, 32, M - 1]
LONELY_SAMPLES = lambda N: [0, 31, 32, 63, 64, N - 1]
_INPUTS, _MODELS = {}, {}


def make_input(family, M, N, miss, seed=0):
    """(G int8 [M][N], mu f32, sigma f32, keep u8) -- miss: "none", "random" (2 %) or ("lonely", row, sample).  Cached; do not modify."""
    key = (family, M, N, miss, seed)
    if key in _INPUTS:
        return _INPUTS[key]
    rng = np.random.default_rng([seed, M, N, sorted(FAMILIES).index(family) if family in FAMILIES else 9])
    p = rng.uniform(0.05, 0.5, size=M)
    rare = M - 3
    if family == "spread":
        p[rare] = 1e-4
    G = (rng.random((M, N)) < p[:, None]).astype(np.int8) + (rng.random((M, N)) < p[:, None]).astype(np.int8)
    if family == "spread":
        G[rare, ::17] = 1; G[rare, 5::34] = 2                       # (the rare allele is seen: the row's w and 2w enter the products)
    mu = (2 * p).astype(np.float32)
    sigma = np.sqrt(2 * p * (1 - p)).astype(np.float32)
    if family == "centred":
        mu = rng.uniform(0.01, 1.9, size=M).astype(np.float32)
    if family == "pow2":
        sigma = (2.0 ** -rng.integers(0, 6, size=M)).astype(np.float32)
        sigma[M // 3] = 1.0 / 32                                    # (vmax = 2^11 whatever the draw)
    if family == "tie":                                             # S = 1/2: c / S = 4.5 and 12.5 in rows 1 and 3
        mu = np.resize(np.array([2.0 ** 20, 2.25, 0.75, 6.25, 1.0, 0.5], np.float32), M)
    if miss == "random":
        G[rng.random((M, N)) < 0.02] = MISSING
    elif miss != "none":
        G[miss[1], miss[2]] = MISSING
    keep = np.ones(M, np.uint8)
    if M >= 12 and family != "tie":
        if miss == "random":
            G[BAD_ROW, N // 3] = MISSING                            # (the row that is not kept holds a missing call too)
        G[BAD_ROW, N // 2] = 3; sigma[BAD_ROW] = np.nan; keep[BAD_ROW] = 0
        sigma[TINY_ROW] = 1e-10
        mu[ZERO_MU_ROW] = 0.0
    for x in (G, mu, sigma, keep):
        x.setflags(write=False)
    _INPUTS[key] = (G, mu, sigma, keep)
    return _INPUTS[key]


def model_of(family, M, N, miss, scaling, keep_name="every row", seed=0):
    """the cached model of one case (shared by the storage parameter, the CPU tests and the teeth)"""
    key = (family, M, N, miss, scaling, keep_name, seed)
    if key not in _MODELS:
        G, mu, sigma, keep = make_input(family, M, N, miss, seed)
        _MODELS[key] = grm_model(G, mu, sigma, keep_of(M, keep, keep_name), scaling)
    return _MODELS[key]


def keep_of(M, base, name):
    return dict(edge_keeps(M))[name] & base


EDGE_CASES = [(M, 65) for M in EDGE_M] + [(33, N) for N in EDGE_N]
FAMILY_CASES = [(f, miss) for f in FAMILIES for miss in ("none", "random")]
LONELY_CASES = [(M, row, s) for M in (33, 4097) for row in LONELY_ROWS(M) for s in LONELY_SAMPLES(129)]
STREAM_M, TWO_RANK_M, BIG_M, BIG_N = 4097 + 3072, 4097, 4097, 129


def every_case():
    """(label, family, M, N, miss, scaling, keep name) of every resident, streamed, sharded and band case of this module"""
    out = []
    for M, N in EDGE_CASES:
        for name, _ in edge_keeps(M):
            out += [(f"edge {M}x{N} {name} {s}", "generic", M, N, "random", s, name) for s in ("standardized", "centred")]
    out += [(f"{f} {miss}", f, BIG_M, BIG_N, miss, FAMILIES[f], "every row") for f, miss in FAMILY_CASES]
    for M, row, s in LONELY_CASES:
        out += [(f"lonely {M} ({row}, {s}) {sc}", "generic", M, BIG_N, ("lonely", row, s), sc, "every row") for sc in ("standardized", "centred")]
    out += [(f"streamed {sc}", "generic", STREAM_M, BIG_N, "random", sc, "every row") for sc in ("standardized", "centred")]
    out += [(f"two ranks {f}", f, TWO_RANK_M, BIG_N, "random", "standardized", "every row") for f in ("generic", "spread")]
    out += [("tie", "tie", 33, 65, "random", "centred", "every row")]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------------------------------------------------------------
def test_model_equals_python_ints():
    for family, scaling in (("generic", "standardized"), ("spread", "standardized"), ("centred", "centred"), ("pow2", "standardized")):
        G, mu, sigma, keep = make_input(family, 40, 9, "random", seed=3)
        G = G.copy(); G[[0, 13, 39], [1, 4, 8]] = MISSING                   # (9 samples at 2 % would hold few missing calls)
        S, I, npairs, big = grm_model_python_ints(G, mu, sigma, keep, scaling)
        for bits in (None, 14):
            mdl = grm_model(G, mu, sigma, keep, scaling, limb_bits=bits)
            assert mdl.S == S and mdl.big == big and mdl.K == 39
            for a in range(9):
                for b in range(a + 1):
                    assert int(mdl.I[a, b]) == I[a][b] and int(mdl.npairs[a, b]) == npairs[a][b], (family, a, b)
                    assert mdl.grm[a, b] == float(I[a][b]) * S / 39 and mdl.grm[b, a] == mdl.grm[a, b]


def test_scale_search_and_rounding():
    """S on both sides of the edge of the search, llround against rint on exact ties, and the families' scales"""
    assert pick_scale(2.0 ** 11) == 2.0 ** -30 and pick_scale(QMAX * 2.0 ** -31) == 2.0 ** -31 and pick_scale(0.0) == 1.0
    assert pick_scale(np.nextafter(QMAX * 2.0 ** -31, 4096.0)) == 2.0 ** -30
    assert pick_scale(float(QMAX)) == 1.0 and pick_scale(float(QMAX + 1)) == 2.0
    x = np.array([0.0, 0.49999999999999994, 0.5, 1.5, 2.5, 4.5, 12.5, 2.0 ** 41 + 0.5, 3.25])
    assert round_half_away(x).tolist() == [0, 0, 1, 2, 3, 5, 13, 2 ** 41 + 1, 3]
    assert round_half_even(x).tolist() == [0, 0, 0, 2, 2, 4, 12, 2 ** 41, 3]
    want = {"centred": -40, "pow2": -30, "generic": -37, "spread": -28}
    for f, miss in FAMILY_CASES:
        mdl = model_of(f, BIG_M, BIG_N, miss, FAMILIES[f])
        assert mdl.S == 2.0 ** want[f], (f, mdl.S)
        twice = float(np.mean(mdl.q["w2"][mdl.q["w"] > 0] != 2 * mdl.q["w"][mdl.q["w"] > 0]))
        if f in ("centred", "pow2"):
            assert twice == 0.0
        if f == "generic":
            assert 0.35 <= twice <= 0.65 and all(np.any((mdl.q["w2"] >> (7 * d)) & 127) for d in range(DIGITS))
    assert model_of("tie", 33, 65, "random", "centred").S == 0.5


def test_every_case_is_in_the_exact_regime():
    biggest = 0
    for label, family, M, N, miss, scaling, keep_name in every_case():
        big = model_of(family, M, N, miss, scaling, keep_name).big
        assert big < 2 ** 53, (label, math.log2(big))
        biggest = max(biggest, big)
    print(f"{len(every_case())} cases, the largest big = 2^{math.log2(biggest):.2f}")


def test_model_within_quantisation_bar():
    from test_gpu_grm import ref_grm
    worst = (0.0, None)
    for label, family, M, N, miss, scaling, keep_name in every_case():
        G, mu, sigma, base = make_input(family, M, N, miss)
        keep = keep_of(M, base, keep_name)
        keepb = keep.astype(bool)
        mdl = model_of(family, M, N, miss, scaling, keep_name)
        with np.errstate(all="ignore"):
            ref, ref_np = ref_grm(G, dict(mu=mu, sigma=sigma, keep=keep), scaling)
        assert np.array_equal(ref_np, mdl.npairs), label
        X = G[keepb]; m = (X == MISSING).astype(np.float64); ga = np.where(X == MISSING, 0, X).astype(np.float64)
        K = mdl.K
        n_ab = ga.T @ ((ga > 0) + m) + m.T @ (ga + m) + ga.sum(0)[:, None] + ga.sum(0)[None, :] + K + m.sum(0)[:, None] + m.sum(0)[None, :]
        r, b = scale_rb(mu, sigma, keepb, scaling)
        Z = np.abs(np.where(X == MISSING, 0.0, X * r[keepb][:, None] + b[keepb][:, None]))
        bar = mdl.S / (2 * K) * n_ab + U64 * np.abs(mdl.grm) + (K + 4) * U64 * (Z.T @ Z) / K
        il = np.tril_indices(N)
        d = np.abs(mdl.grm - ref)[il]
        frac = float(np.max(d / bar[il]))
        assert np.all(d <= bar[il]), (label, frac)
        if frac > worst[0]:
            worst = (frac, label)
    RECORD["quant"] = worst[0]
    print(f"model against ref_grm: the largest fraction of the bar {worst[0]:.3f} ({worst[1]})")


PLANE_MUTANTS = {f"drop plane {d} of {t}": {"drop_plane": (t, d)} for t in TABLES for d in range(DIGITS)}
MUTANTS = dict(PLANE_MUTANTS, **{
    "2 q(w) for q(2w)": {"w2_is_twice_w": True}, "sides swapped": {"swap_sides": True},
    "selector: w plane for g' = 2": {"two_takes_w": True}, "selector: 2w plane for g' = 1": {"one_takes_2w": True},
    "c dropped on the a side": {"drop_c_on_a_side": True}, "c dropped on the b side": {"drop_c_on_b_side": True},
    "e where c belongs": {"e_for_c": True},
    "missing path skipped, only the row side missing": {"skip_when_only_a_side_missing": True},
    "missing path skipped, only the column side missing": {"skip_when_only_b_side_missing": True},
    "u from q(w)": {"u_from_w": True}, "beta without the last kept row": {"beta_short": True},
    "v without the keep mask": {"v_without_keep": True}, "NPAIRS without the keep mask": {"npairs_without_keep": True},
    "S one step too large": {"s_steps": 1}})
SYMMETRIC_FAMILIES = ("centred", "pow2")
NEEDS_MISSING = ("c dropped on the a side", "c dropped on the b side", "e where c belongs", "v without the keep mask", "NPAIRS without the keep mask")
BALLOT = ("missing path skipped, only the row side missing", "missing path skipped, only the column side missing")
# planes that hold no nonzero digit in any kept row of a family's 4097 x 129 cases (S = 2^-28 leaves c, e <= 2^30 in ``spread``; in ``pow2``
# w is a power of two between 2^30 and 2^40 in units of S; in ``centred`` w = 2^40 and c = mu >= 2^-7 is a multiple of 2^-30 = 2^10 S)
ZERO_PLANES = {"spread": {("c", 5), ("e", 5)},
               "pow2": {("w", 0), ("w", 1), ("w", 2), ("w", 3), ("w2", 0), ("w2", 1), ("w2", 2), ("w2", 3)},
               "centred": {(t, d) for t in ("w", "w2") for d in range(5)} | {("c", 0)}, "generic": set()}


def _moves(name, mut, family, M, N, miss, scaling, keep_name="every row"):
    G, mu, sigma, base = make_input(family, M, N, miss)
    base_m = model_of(family, M, N, miss, scaling, keep_name)
    mm = grm_model(G, mu, sigma, keep_of(M, base, keep_name), scaling, mut=mut)
    il = np.tril_indices(N)
    return not np.array_equal((mm.npairs if name.startswith("NPAIRS") else mm.grm)[il], (base_m.npairs if name.startswith("NPAIRS") else base_m.grm)[il])


def test_teeth():
    """every mutant moves a bit of the lower triangle in at least one case of every family it can touch"""
    M, N = BIG_M, BIG_N
    for f in FAMILIES:                                  # the planes that cannot be touched are exactly ZERO_PLANES
        zero = {(t, d) for t in TABLES for d in range(DIGITS)
                if not any(np.any((model_of(f, M, N, miss, FAMILIES[f]).q[t] >> (7 * d)) & 127) for miss in ("none", "random"))}
        assert zero == ZERO_PLANES[f], (f, sorted(zero))
    for name, mut in MUTANTS.items():
        for f in FAMILIES:
            sc = FAMILIES[f]
            if name in BALLOT:
                continue
            cases = [miss for miss in ("none", "random") if not (miss == "none" and (name in NEEDS_MISSING or mut.get("drop_plane", "w")[0] in "ce"))]
            moved = [_moves(name, mut, f, M, N, miss, sc) for miss in cases]
            if name in ("2 q(w) for q(2w)", "sides swapped") and f in SYMMETRIC_FAMILIES:
                assert not any(moved), (name, f)        # q(2w) = 2 q(w) on every row: the product is symmetric, nothing can move
            elif "drop_plane" in mut and mut["drop_plane"] in ZERO_PLANES[f]:
                assert not any(moved), (name, f)        # the plane is zero throughout the family
            elif name == "v without the keep mask" and f != "centred":
                assert not any(moved), (name, f)        # a row that is not kept has b = 0 under the standardized scaling
            else:
                assert any(moved), (name, f)
    # v and NPAIRS without the keep mask: the keeps that drop rows holding missing calls
    for name in ("v without the keep mask", "NPAIRS without the keep mask"):
        assert _moves(name, MUTANTS[name], "generic", 4097, 65, "random", "centred", "last block dropped"), name
        assert _moves(name, MUTANTS[name], "generic", 33, 129, "random", "centred", "one row"), name
    assert not _moves("v", MUTANTS["v without the keep mask"], "generic", 4097, 65, "random", "standardized", "last block dropped")
    # the ballot mutants: one missing call in the matrix.  The row-side one needs a column group below the missing sample's own, the
    # column-side one a row group above it; at least one position of each row does, at both row counts
    for name in BALLOT:
        for Mr in (33, 4097):
            for row in LONELY_ROWS(Mr):
                hit = {s: [_moves(name, MUTANTS[name], "generic", Mr, N, ("lonely", row, s), sc) for sc in ("standardized", "centred")]
                       for s in LONELY_SAMPLES(N)}
                can = {s: (s >= 32) if "row side" in name else (s < 128) for s in hit}
                for s in hit:
                    assert all(hit[s]) if can[s] else not any(hit[s]), (name, Mr, row, s)
    # every other mutant of the missing path moves every lonely case it can touch too (the plane-level teeth stay on these)
    for name in ("c dropped on the a side", "c dropped on the b side", "e where c belongs"):
        assert all(_moves(name, MUTANTS[name], "generic", 33, N, ("lonely", row, 32), "standardized") for row in LONELY_ROWS(33)), name


def test_half_even_rounding_shows_on_the_tie_case():
    G, mu, sigma, keep = make_input("tie", 33, 65, "random")
    S, q = quantise(mu, sigma, keep, "centred")
    assert S == 0.5 and q["c"][1] == 5 and q["c"][3] == 13 and q["c"][2] == 2
    _, qe = quantise(mu, sigma, keep, "centred", rounding=round_half_even)
    assert qe["c"][1] == 4 and qe["c"][3] == 12 and qe["c"][2] == 2
    il = np.tril_indices(65)
    assert not np.array_equal(grm_model(G, mu, sigma, keep, "centred", mut={"rounding": round_half_even}).grm[il], model_of("tie", 33, 65, "random", "centred").grm[il])


# ---------------------------------------------------------------------------------------------------------------------------------
# device tests
# ---------------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _standardize(e, mu, sigma, keep):
    e.set_standardization(mu, sigma, keep)
    st = e.get_standardization()
    assert _same(st["mu"], mu) and _same(st["sigma"], sigma) and np.array_equal(st["keep"].astype(np.uint8), keep)


def _resident(store, family, M, N, miss, scalings, keeps=("every row",)):
    G, mu, sigma, base = make_input(family, M, N, miss)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.upload_genotypes_i8(G)
        for name in keeps:
            keep = keep_of(M, base, name)
            _standardize(e, mu, sigma, keep)
            for scaling in scalings:
                mdl = model_of(family, M, N, miss, scaling, name)
                tri, npt = e.grm(scaling, rows=(0, N), npairs=True)
                assert check_device(tri, npt, mdl, flush_groups(M), (store, family, M, N, miss, name, scaling)) == "exact"


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["int8", "2bit"])
@pytest.mark.parametrize("M,N", EDGE_CASES)
def test_edge_shapes_equal_the_model(store, M, N):
    _resident(store, "generic", M, N, "random", ("standardized", "centred"), [name for name, _ in edge_keeps(M)])


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["int8", "2bit"])
@pytest.mark.parametrize("family,miss", FAMILY_CASES + [("tie", "random")])
def test_families_equal_the_model(store, family, miss):
    if family == "tie":
        _resident(store, "tie", 33, 65, miss, ("centred",))
    else:
        _resident(store, family, BIG_M, BIG_N, miss, (FAMILIES[family],))


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["int8", "2bit"])
@pytest.mark.parametrize("M,row,sample", LONELY_CASES)
def test_one_missing_call_equals_the_model(store, M, row, sample):
    _resident(store, "generic", M, BIG_N, ("lonely", row, sample), ("standardized", "centred"))


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["int8", "2bit"])
@pytest.mark.parametrize("panel_rows", [8192, 3072, 1000])
def test_streamed_panels_equal_the_model(store, panel_rows):
    """panels of a multiple of the flush group, of a multiple of 32 rows that is not one, and of a row count gpca_stream_open rounds up"""
    M, N = STREAM_M, BIG_N
    G, mu, sigma, keep = make_input("generic", M, N, "random")
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), M, N, panel_rows=panel_rows, ring_slots=2, fused=False)
        pr = e.stream_info()["panel_rows"]
        assert pr % 128 == 0 and pr >= min(panel_rows, M)
        _standardize(e, mu, sigma, keep)
        for scaling in ("standardized", "centred"):
            tri, npt = e.grm(scaling, rows=(0, N), npairs=True)
            mdl = model_of("generic", M, N, "random", scaling)
            assert check_device(tri, npt, mdl, flush_groups(M, pr), (store, panel_rows, scaling)) == "exact"


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["generic", "spread"])
def test_two_ranks_equal_the_model(family):
    """the rare row of ``spread`` (row M - 3) is on rank 1, so rank 0 learns its scale from the first exchange"""
    from test_gpu_grm import _two_ranks
    M, N = TWO_RANK_M, BIG_N
    G, mu, sigma, keep = make_input(family, M, N, "random")
    assert gpca.shard_rows(M, 2, 1)[0] <= M - 3
    if family == "spread":
        first = gpca.shard_rows(M, 2, 0)
        sl = slice(*first)
        assert quantise(mu[sl], sigma[sl], keep[sl], "standardized")[0] < model_of(family, M, N, "random", "standardized").S
    mdl = model_of(family, M, N, "random", "standardized")
    il = np.tril_indices(N)
    P = sum(flush_groups(b - a) for a, b in (gpca.shard_rows(M, 2, r) for r in range(2)))
    for res in _two_ranks(G, dict(mu=mu, sigma=sigma, keep=keep), "standardized"):
        assert not isinstance(res, Exception), res
        g, n = res
        assert check_device(g[il], n[il], mdl, P, ("two ranks", family), ranks=2) == "exact"


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_band_off_a_tile_multiple_equals_the_model(store):
    M, N, rows = BIG_M, BIG_N, (65, 129)
    G, mu, sigma, keep = make_input("generic", M, N, "random")
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        e.upload_genotypes_i8(G)
        _standardize(e, mu, sigma, keep)
        for scaling in ("standardized", "centred"):
            tri, npt = e.grm(scaling, rows=rows, npairs=True)
            assert check_device(tri, npt, model_of("generic", M, N, "random", scaling), flush_groups(M), (store, "band", scaling), rows=rows) == "exact"
