"""The EigenSNP stage kernels (gpca_copy_rows, gpca_set_sample_mask, gpca_set_condensed_basis, gpca_rsvd_condensed, gpca_refine) held to
bars derived from their arithmetic, at the shapes where k_bd_expand, k_bd_reduce, k_rightmul_inplace_f32, k_mask_rows, launch_omega over
feature indices and the zmode = 1 eigen step can go wrong.  Style and helpers of test_gpu_exact_pass.py and test_gpu_k1_pass.py.

NOTATION.  A = the standardised kept rows ((g - mu) / sigma in f64 from the uploaded bytes and the CPU's mu, sigma; the device's are held
to them by ``device_stats``), Wd = the dense M x R form of the caller's (W, feat0, cmax), C = Wd^T A (R x N), S = scores(f64 = True),
sv_c^2 = eigenvalue_c (N - 1), l = k + oversample, L = 32 or 64, u32 = 2^-24, u64 = 2^-53, EIG = 1e-12 (what test_gpu_parity.py holds the device
eigen solver to, of the largest eigenvalue).  Nothing read back is trusted: every right-hand side is recomputed from the bytes.

I1, THE FORWARD PRODUCT (stage_AQ, k_bd_reduce, the Gram of P, the eigen step; any q, any oversample, any hidden Q).  The device forms
P = C Q + dP, P^T P = V diag(sv^2) V^T, S = Q V_k diag(sv).  So Z = C S (f64, CPU) = (P - dP) V_k diag(sv) and, with e = |dP v|_2 for a unit v,
    | (Z^T Z)_cd / (sv_c^2 sv_d^2) - [c = d] |  <=  e / sv_c + e / sv_d + e^2 / (sv_c sv_d) + the f64 terms           (``i1_bar``)
  dP = Wd^T dB + the fma chain of k_bd_reduce:  e <= | ( sum_i |Wd_if| (|dB_i.|_2 + u64 (nb + 1) |A_i.|_2) )_f |_2, nb = the longest row range
    of a block (one fma per row), |B_i.|_2 <= |A_i.|_2 (Q has orthonormal columns).  |dB_i.|_2 is K1's bar of test_gpu_k1_pass.py: for every
    column c,  k1_bar_ic >= |dB_i.|_2 / sv_c, so |dB_i.|_2 <= min_c sv_c k1_bar_ic -- its oversample = 0 branch (Q's row norms are those of
    S / sv) where k = l, its worst-case branch otherwise.
  f64: the Gram of P (R terms per element, |dG|_F <= R u64 |P|_F^2 = R u64 sum_j sv_j^2) and the eigen step (EIG sv_0^2), both over sv_c sv_d;
    the scores' product of l terms, carried by C: u64 (l + 2) sqrt(l) smax(C) (1 / sv_c + 1 / sv_d); this file's own Z and Z^T Z: 2 (N + R) u64.
I2, THE BACKWARD PRODUCT (launch_omega over features, k_bd_expand, launch_scale_rows, K2, stage_orth; q = 0, oversample = 0, k = l).
  span(S) = span(Y), Y = A^T T + dY, T = f32(Wd Omega_R), Omega_R = the Philox normals over (feature, column) the oracle draws in f64,
  stored as f32 with r = 1, b = 0 (launch_omega writes Tb = rs * (float) z, then k_f32_to_f64).  With Pn an orthonormal basis of span(S),
    | ((I - Pn Pn^T) Y_true)_.j |_2  <=  | bar_.j |_2 + count u64 |Y_true_.j|_2,        Y_true = C^T Omega_R                  (``i2_bar``)
  bar_nj, exact modes: ``bounds(exact_pass_model(T), generic = True)`` against ref_project (K2's own bar for the model T) plus the store of
    k_bd_expand carried by A: (u32 + (cmax + 1) u64) sum_i |A_in| |T_ij| (one f32 rounding after a chain of cmax f64 fmas).
  bar_nj, GPCA_PREC_F32_MFMA (k_gtt_f32: one f32 accumulator per (sample, column) and wave, a chain of rows_per_wave fmas, gtt_plan of
    plan_math.h restated in ``f32_k2_chain``; the waves' partials and c fold in f64): u32 ((chain + 3) sum_i g_in |r_i T_ij| + (64 + 4)
    sum_i |b_i T_ij|) (1 + 8 u32): r, r T and the store of T round once each, b twice, b T once, its 64-row partial at most 64 times.
  count = 2 l sqrt(l) cond(Y_true) + (l + 2) sqrt(l) + 2 N: two rounds of Y R^-1 (l terms against a factor of that condition), the scores'
    product, this file's own sums.  Checked before anything is launched: R >= 2 l and cond(Y_true)^2 u64 < 1.
I3, THE SCORES SIDE OF gpca_refine (second pass S = A^T L, its Gram, the zmode = 1 eigen step, launch_scores).  loadings = f32(L W),
  scores = (A^T L + dS) W with the same W, so scores_nc = sum_i A_in loadings_ic within
    sqrt(k) e_n + u32 sum_i |A_in loadings_ic| + u64 (N + k + 2) (|scores_n.|_2 + sum_i |A_in loadings_ic|)                    (``i3_bar``)
  e_n bounds every |dS_nj|: L = loadings W^T is hidden, |L_ij| <= |loadings_i.|_2 (1 + 2 u32), so e_n is the exact-pass truth bar
    (``bounds``, generic) of the one-column model T_i = |loadings_i.|_2 -- column maximum, sum_i g |Ta|, sum_i |Tb| all dominate L's; on
    GPCA_PREC_F32_MFMA the chain bar of I2 on the same column.  And  | (S^T S)_cd / (sv_c sv_d) - [c = d] | <= (u64 (2 N + 4 (k + 2))
    sum_j sv_j^2 + EIG sv_0^2) / (sv_c sv_d): the Gram's N terms, the product's k, this file's own N, the eigen step.
I4, THE LOCAL STAGE.  A gpca_copy_rows child of a row range, keep a strict subset of it, gpca_set_sample_mask, gpca_rsvd, gpca_transform:
  the features of ALL samples through ``check_against_bars`` (model and truth) against the child's own f32 loadings, the masked fit's
  loadings through ``k1_bar(mask = ...)``.  Exact modes (the exact-pass model is theirs).

TEETH (CPU, unmarked).  ``simulate_condensed`` / ``simulate_refine`` run the device recipe in numpy: K1 by ``simulate_k1``, K2 by
``exact_pass_model``, the two bd kernels restated (``bd_expand``, ``bd_reduce``; stale rows of dP stay as on the device), f64 QR for
CholeskyQR2.  The unmutated simulator and oracle.eigensnp_global_and_refine sit inside every bar; each mutant of ``MUTANTS`` leaves the bar
of its identity on the device tests' own generator and shapes (a non-finite result counts as outside).

NOT REACHED, AND WHY.  I2 at R = l is blind (every expand defect stays inside span(C^T) = span(S)), hence R >= 2 l; it sees only what
leaves span(S), I1 only what breaks P = C Q: a fault common to both products of a call (a wrong A) is the parity tests' business.  Omega_R
kept in f64 (mutant ``omega_f64``, and the f64 oracle) moves T by half an f32 ulp at random, under the u32 terms of K2's bar that add up
absolute values: invisible, 0.0003 of the bar on the CPU.  With oversample > 0 the K1 term is the worst-case branch, as in the K1 module.
The f32 K2 chain term grows with rows_per_wave; at these shapes it is 32.  The Philox subset draw and the reference crate's own output are
out of scope.

Measured on the CPU (the teeth, int8 / 2-bit digit counts 4 / 3), the largest fraction of each bar; each test prints its own with -s:
    unmutated simulator  I1 0.00074 / 0.00015, I2 0.0026 / 0.024, I3 scores 0.00055 / 0.0052 and Gram 0.00095, I4 model against truth 0.016 / 0.11
    the f64 oracle       I1 0.00056, I2 0.00065, I3 0.00013 and 0.0013, I4 0.0083;  the weakest mutant: last_unit_out at k = 33, 24 x its bar
Measured on one MI355X, the largest fraction of each bar over every case and element (int8 / 2-bit 3 planes / 2-bit 4 planes / f32 MFMA on
int8 and on 2-bit rows; records, not thresholds):
    I1  0.092 / 0.039 / 0.092 / 0.00035 / 0.00035           I2  0.0088 / 0.096 / 0.0088 / 0.0083 / 0.0083
    I3  scores 0.0050 / 0.051 / 0.0050 / 0.0024 / 0.0024,  Gram 0.00088 / 0.0011 / 0.00088 / 0.00087 / 0.00087
    I4  loadings 0.21 / 0.12 / 0.21,  features against the model 0.0029 / 0.0027 / 0.0029, against the truth 0.056 / 0.18 / 0.056
One value-only defect compiled into k_bd_reduce on a scratch copy (the c stride off: features c >= 8 of a block never written), run once:
33 of the 35 I1 cases with cmax > 8 went red (cmax = 9, 50, 64; the two that stayed green are cmax = 9, l = 15 on GPCA_PREC_F32_MFMA, where
one missing feature of nine stays under that mode's chain term), every cmax <= 8 case stayed green, and
test_condensed_global_pca_and_refinement (cmax = 4, 1e-4) stayed green beside them on all three of its modes."""
import numpy as np
import pytest

from test_gpu_exact_pass import bounds, check_against_bars, exact_pass_model, ref_project
from test_gpu_k1_pass import (EXACT, MODES, U32, U64, case_inputs, check, device_stats, k1_bar, k1_truth, open_engine,
                              orth_as_cholqr, refine_start, simulate_k1)

EIG = 1e-12


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def make_layout(name, M, cmax, l=0, seed=0):
    """(W [M][cmax] f32, feat0 [M] i32, R, nb): blocks as (rows, features); feat0 ascends in the order listed.  QC-dropped rows inside a block
    keep their coefficients (their r = b = 0 takes them out on the device, a zero row of A here)."""
    if name in ("mixed", "short_last"):
        assert M == 4097
        single, half = (np.array([5]), 1), max(1, cmax // 2)
        ia, ib = (np.arange(100, 900, 2), cmax), (np.arange(101, 900, 2), cmax)              # rows of one inside the other's range
        holes = np.arange(1000, 2000)
        holes = (holes[holes % 5 != 0], cmax)                                                # rows with feat0 = -1 inside the range
        if name == "mixed":                                                                 # the short block before larger ones
            blocks = [single, (np.arange(10, 41), half), ia, ib, holes, (np.arange(2100, M), cmax)]
        else:                                                                               # ... and last: feat0 + cmax > R
            blocks = [single, ia, ib, holes, (np.arange(2100, 3500), cmax), (np.arange(3600, M), half)]
    elif name == "one_block":
        blocks = [(np.arange(M), cmax)]
    elif name == "exact_R":                                                                 # R = l; the last block is the short one
        nblk = -(-l // cmax)
        edges = np.linspace(0, M, nblk + 1).astype(int)
        blocks = [(np.arange(edges[i], edges[i + 1]), cmax if i < nblk - 1 else l - cmax * (nblk - 1)) for i in range(nblk)]
    else:                                                                                   # "small": 33 rows, R < 32
        assert name == "small" and M == 33 and cmax <= 13
        blocks = [(np.array([0]), 1), (np.arange(1, 7), min(cmax, 2)), (np.arange(7, M, 2), cmax), (np.arange(8, M, 2), cmax)]
    rng = np.random.default_rng(seed + cmax)
    W, feat0, R = np.zeros((M, cmax), np.float32), np.full(M, -1, np.int32), 0
    for rows, c in blocks:
        assert 1 <= c <= min(cmax, len(rows))
        W[rows, :c] = (rng.standard_normal((len(rows), c)) / np.sqrt(len(rows))).astype(np.float32)
        feat0[rows] = R
        R += c
    nb = max(int(rows[-1] - rows[0] + 1) for rows, _ in blocks)
    return W, feat0, R, nb


def dense_basis(W, feat0, R):
    M, cmax = W.shape
    Wd = np.zeros((M, R + cmax))
    for i in np.flatnonzero(feat0 >= 0):
        Wd[i, feat0[i]:feat0[i] + cmax] += W[i]
    assert not np.any(Wd[:, R:]), "coefficients past the block's own features must be the zero padding"
    return Wd[:, :R]


def standardized(G, mu, sigma, rows):
    return (G[rows].astype(np.float64) - mu[rows].astype(np.float64)[:, None]) / sigma[rows].astype(np.float64)[:, None]


def omega_f32(oracle, R, l, seed):
    """Omega_R as the device holds it: the f64 draw rounded to f32 (launch_omega with r = 1, b = 0), widened again"""
    return oracle.omega(R, l, seed).astype(np.float32).astype(np.float64)


def f32_k2_chain(M, N, target=2048):
    """rows_per_wave of gtt_plan (plan_math.h) at the default wave target: the length of k_gtt_f32's fma chain"""
    Mpad, Npad = (M + 127) // 128 * 128, (N + 255) // 256 * 256
    W = min(max(target // (Npad // 256), 1), Mpad // 32)
    return (-(-Mpad // W) + 31) // 32 * 32


def frac_of(d, bar):
    """largest |d| / bar; a non-finite element or one over a zero bar counts as infinitely far out"""
    d, bar = np.abs(np.asarray(d, np.float64)), np.asarray(bar, np.float64)
    if not (np.all(np.isfinite(d)) and np.all(np.isfinite(bar))):
        return np.inf
    return float(np.max(np.where(bar > 0, d / np.where(bar > 0, bar, 1), np.where(d > 0, np.inf, 0)), initial=0))


def held(d, bar, what):
    f = frac_of(d, bar)
    print(f"{what}: {f:.3g} of the bar")
    assert f <= 1, f"{what}: {f:.3g} of the bar"
    return f


# ---- the bars ----------------------------------------------------------------------------------------------------------------------------
def i1_bar(G, mu, sigma, rows, ulps, Wd, nb, S, sv, sv_all, l, nd):
    """(E = Z^T Z / (sv_c^2 sv_d^2) - I, its bar), both [k][k]"""
    S, sv, sv_all = np.asarray(S, np.float64), np.asarray(sv, np.float64), np.asarray(sv_all, np.float64)
    N, k = S.shape
    A = standardized(G, mu, sigma, rows)
    Cm = Wd[rows].T @ A
    R = Cm.shape[0]
    Z = Cm @ S
    with np.errstate(all="ignore"):
        E = (Z.T @ Z) / np.outer(sv ** 2, sv ** 2) - np.eye(k)
        truth = k1_truth(G, mu, sigma, rows, S, sv)
        kb = k1_bar(G, mu, sigma, rows, S, sv, l, nd, truth, None, ulps)
        dB = np.min(kb * sv[None, :], axis=1) + U64 * (nb + 1) * np.sqrt(np.sum(A * A, axis=1))
        e = float(np.linalg.norm(np.abs(Wd[rows]).T @ dB))
        t = e / sv
        smax = float(np.linalg.svd(Cm, compute_uv=False)[0])
        bar = t[:, None] + t[None, :] + np.outer(t, t)
        bar += (U64 * R * np.sum(sv_all ** 2) + EIG * sv_all[0] ** 2) / np.outer(sv, sv)
        bar += U64 * (l + 2) * np.sqrt(l) * smax * (1 / sv[:, None] + 1 / sv[None, :]) + 2 * (N + R) * U64
    return E, bar


def k2_column_bar(G, mu, sigma, rows, T, nd, chain):
    """[N][cols]: what one K2 pass Y = A^T T can be off the f64 truth by, T [M][cols] f32 (zero outside the kept rows)"""
    if nd:
        return bounds(exact_pass_model(G, mu, sigma, T, nd), True)[1]
    r = 1.0 / sigma[rows].astype(np.float64)
    b = np.abs(mu[rows].astype(np.float64)) * r
    Tk = np.abs(T[rows].astype(np.float64))
    return U32 * ((chain + 3) * (G[rows].astype(np.float64).T @ (r[:, None] * Tk)) + 68 * np.sum(b[:, None] * Tk, axis=0)[None, :]) * (1 + 8 * U32)


def i2_truth(G, mu, sigma, rows, Wd, Om, l):
    """(Y_true [N][l], T_true [M][l] f64, cond(Y_true)) -- and the two conditions of the identity"""
    Tt = Wd @ Om
    Y = standardized(G, mu, sigma, rows).T @ Tt[rows]
    cond = float(np.linalg.cond(Y))
    assert Wd.shape[1] >= 2 * l, "I2 is blind below R = 2 l"
    assert cond ** 2 * U64 < 1, "CholeskyQR needs cond(Y)^2 u64 < 1"
    return Y, Tt, cond


def i2_bar(G, mu, sigma, rows, cmax, S, Y, Tt, cond, nd):
    """(per-column |(I - Pn Pn^T) Y_true|_2, its bar), both [l]"""
    N, l = Y.shape
    kept = np.zeros(G.shape[0], bool); kept[rows] = True
    T32 = np.where(kept[:, None], Tt, 0.0).astype(np.float32)
    el = k2_column_bar(G, mu, sigma, rows, T32, nd, f32_k2_chain(G.shape[0], N))
    el = el + (U32 + (cmax + 1) * U64) * (np.abs(standardized(G, mu, sigma, rows)).T @ np.abs(Tt[rows]))
    count = 2 * l * np.sqrt(l) * cond + (l + 2) * np.sqrt(l) + 2 * N
    bar = np.linalg.norm(el, axis=0) + count * U64 * np.linalg.norm(Y, axis=0)
    if not np.all(np.isfinite(S)):
        return np.full(l, np.inf), bar
    Pn, _ = np.linalg.qr(np.asarray(S, np.float64))
    return np.linalg.norm(Y - Pn @ (Pn.T @ Y), axis=0), bar


def i3_bars(G, mu, sigma, rows, S, load, sv, nd):
    """(scores - A^T loadings and its bar [N][k], S^T S / (sv_c sv_d) - I and its bar [k][k])"""
    S, load, sv = np.asarray(S, np.float64), np.asarray(load, np.float32).astype(np.float64), np.asarray(sv, np.float64)
    N, k = S.shape
    M = G.shape[0]
    A = standardized(G, mu, sigma, rows)
    model = A.T @ load
    absm = np.abs(A).T @ np.abs(load)
    T = np.zeros((M, 1), np.float32)
    T[rows, 0] = (np.sqrt(np.sum(load * load, axis=1)) * (1 + 4 * U32)).astype(np.float32)      # >= |L_ij| (1 + 2 u32), rounded to f32 once more
    e = k2_column_bar(G, mu, sigma, rows, T, nd, f32_k2_chain(M, N))[:, 0]
    bar = np.sqrt(k) * e[:, None] + U32 * absm + U64 * (N + k + 2) * (np.sqrt(np.sum(S * S, axis=1))[:, None] + absm)
    with np.errstate(all="ignore"):
        E = (S.T @ S) / np.outer(sv, sv) - np.eye(k)
        ebar = (U64 * (2 * N + 4 * (k + 2)) * np.sum(sv ** 2) + EIG * sv[0] ** 2) / np.outer(sv, sv)
    return S - model, bar, E, ebar


# ---- the two bd kernels restated, the simulators and their mutants (CPU) -------------------------------------------------------------------
MUTANTS = {"I1": ["reduce_c_lt_8", "reduce_j_lt_32", "short_block_writes_cmax", "reduce_ignores_feat0", "reduce_drops_last_row"],
           "I2": ["expand_first_8", "expand_next_feature", "expand_last_row_zero", "omega_f64"],
           "I3": ["c_left_out", "last_unit_out"], "I4": ["unmasked_zeroed"]}


def bd_blocks(feat0, cmax, R):
    """(bf, row0, row1, cb) per distinct feat0, ascending, as gpca_set_condensed_basis makes them"""
    fs = np.unique(feat0[feat0 >= 0])
    out = []
    for n, f in enumerate(fs):
        ii = np.flatnonzero(feat0 == f)
        nxt = int(fs[n + 1]) if n + 1 < len(fs) else R
        out.append((int(f), int(ii[0]), int(ii[-1]) + 1, min(nxt - int(f), cmax)))
    return out


def bd_expand(W, feat0, cmax, P, mutate=None):
    """out[i][j] = f32( sum_c W[i][c] P[feat0[i] + c][j] ), P [R + 64 + 1][l] with its zero tail"""
    idx = np.flatnonzero(feat0 >= 0)
    out = np.zeros((len(feat0), P.shape[1]))
    for c in range(min(cmax, 8) if mutate == "expand_first_8" else cmax):
        out[idx] += W[idx, c].astype(np.float64)[:, None] * P[feat0[idx] + c + (mutate == "expand_next_feature")]
    if mutate == "expand_last_row_zero":
        out[-1] = 0
    return out.astype(np.float32)


def bd_reduce(W, feat0, cmax, T, R, P, mutate=None):
    """P[bf + c][j] = sum over the block's rows of W[i][c] T[i][j] for c < cb; every other entry of P stays as it was"""
    P = P.copy()
    l = T.shape[1]
    cols = np.arange(min(l, 32) if mutate == "reduce_j_lt_32" else l)
    late = []
    for bf, r0, r1, cb in bd_blocks(feat0, cmax, R):
        ii = np.arange(r0, r1)
        ii = ii[feat0[ii] >= 0] if mutate == "reduce_ignores_feat0" else ii[feat0[ii] == bf]
        if mutate == "reduce_drops_last_row":
            ii = ii[:-1]
        cs = np.arange(min(cb, 8) if mutate == "reduce_c_lt_8" else cb)
        P[np.ix_(bf + cs, cols)] = W[np.ix_(ii, cs)].astype(np.float64).T @ T[np.ix_(ii, cols)].astype(np.float64)
        if mutate == "short_block_writes_cmax" and cb < cmax:
            late.append(np.arange(bf + cb, bf + cmax))
    for rr in late:                                               # (the zero padding of W times T: zeros over the next block's features)
        P[rr] = 0
    return P


def signed(scores):
    sgn = np.sign(scores[np.abs(scores).argmax(axis=0), np.arange(scores.shape[1])]); sgn[sgn == 0] = 1
    return scores * sgn, sgn


def simulate_condensed(oracle, G, mu, sigma, rows, W, feat0, R, k, os_, q, nd, seed, mutate=None):
    """(scores [N][k], sv [l]) as gpca_rsvd_condensed makes them on the exact path"""
    M, cmax = W.shape
    l = k + os_
    kept = np.zeros(M, bool); kept[rows] = True
    P = np.zeros((R + 64 + 1, l))
    P[:R] = oracle.omega(R, l, seed) if mutate == "omega_f64" else omega_f32(oracle, R, l, seed)

    def back(P):
        T = bd_expand(W, feat0, cmax, P, mutate) * kept[:, None]
        return orth_as_cholqr(exact_pass_model(G, mu, sigma, T.astype(np.float32), nd)["Y"])

    def forward(Q, P):
        B = np.zeros((M, l), np.float32)
        B[rows] = simulate_k1(G, mu, sigma, rows, Q, nd, packed=nd == 3)
        return bd_reduce(W, feat0, cmax, B, R, P, mutate)
    Q = back(P)
    for _ in range(q):
        P = forward(Q, P)
        Q = back(P)
    P = forward(Q, P)[:R]
    w, V = np.linalg.eigh(P.T @ P)
    w, V = w[::-1], V[:, ::-1]
    sv = np.sqrt(np.maximum(w, 0))
    return signed((Q @ V[:, :k]) * sv[:k])[0], sv


def simulate_refine(G, mu, sigma, rows, S0, nd, mutate=None):
    """(scores, loadings f32 [n_pca][k], sv) as gpca_refine makes them on the exact path"""
    M = G.shape[0]
    B = simulate_k1(G, mu, sigma, rows, orth_as_cholqr(S0), nd, packed=nd == 3).astype(np.float64)
    Lq = np.zeros((M, S0.shape[1]), np.float32)
    Lq[rows] = orth_as_cholqr(B).astype(np.float32)
    m = exact_pass_model(G, mu, sigma, Lq, nd, mutate="last_unit_out" if mutate == "last_unit_out" else None)
    Y = m["Y"] - (m["c"][None, :] if mutate == "c_left_out" else 0.0)
    w, V = np.linalg.eigh(Y.T @ Y)
    w, V = w[::-1], V[:, ::-1]
    sc, sgn = signed(Y @ V)
    return sc, ((Lq[rows].astype(np.float64) @ V) * sgn).astype(np.float32), np.sqrt(np.maximum(w, 0))


def teeth_inputs(oracle, M, N):
    return case_inputs(oracle, M, N, 1000 * N + M)                # (the device tests' own matrix, built once)


def i1_fraction(inp, lay, sc, sv, l, nd):
    G, mu, sigma, rows = inp
    W, feat0, R, nb = lay
    k = sc.shape[1]
    E, bar = i1_bar(G, mu, sigma, rows, np.zeros(len(rows)), dense_basis(W, feat0, R), nb, sc, sv[:k], sv, l, nd)
    return frac_of(E, bar)


@pytest.mark.parametrize("nd", [3, 4])
def test_i1_rejects_every_reduce_mutant(oracle, nd):
    inp = teeth_inputs(oracle, 4097, 257)
    fr = {}
    for cmax, k, os_, q, muts in ((9, 15, 0, 1, MUTANTS["I1"][:1] + MUTANTS["I1"][2:]), (50, 33, 0, 0, MUTANTS["I1"][:2]), (8, 23, 10, 0, [])):
        lay = make_layout("mixed", 4097, cmax)
        for mut in [None] + muts:
            sc, sv = simulate_condensed(oracle, *inp, *lay[:3], k, os_, q, nd, 5, mutate=mut)
            fr[(cmax, mut)] = i1_fraction(inp, lay, sc, sv, k + os_, nd)
            print(f"I1 nd={nd} cmax={cmax} l={k}+{os_} q={q}: mutant {mut}: {fr[(cmax, mut)]:.3g} of the bar")
    for (cmax, mut), f in fr.items():
        assert (f <= 1) if mut is None else (f > 1), f"I1 cmax={cmax} mutant {mut}: {f:.3g} of the bar"


@pytest.mark.parametrize("nd", [3, 4])
def test_i2_rejects_every_expand_mutant(oracle, nd):
    inp = teeth_inputs(oracle, 4097, 257)
    G, mu, sigma, rows = inp
    fr = {}
    for name, cmax, l in (("mixed", 9, 15), ("short_last", 50, 33)):
        W, feat0, R, _ = make_layout(name, 4097, cmax)
        Y, Tt, cond = i2_truth(G, mu, sigma, rows, dense_basis(W, feat0, R), omega_f32(oracle, R, l, 5), l)
        for mut in [None] + MUTANTS["I2"]:
            sc, _ = simulate_condensed(oracle, G, mu, sigma, rows, W, feat0, R, l, 0, 0, nd, 5, mutate=mut)
            fr[(name, mut)] = frac_of(*i2_bar(G, mu, sigma, rows, cmax, sc, Y, Tt, cond, nd))
            print(f"I2 nd={nd} {name} cmax={cmax} l={l}: mutant {mut}: {fr[(name, mut)]:.3g} of the bar")
    for (name, mut), f in fr.items():
        if mut == "omega_f64":                                     # (NOT REACHED of the module docstring: under the u32 terms of K2's bar)
            assert f <= 1
        else:
            assert (f <= 1) if mut is None else (f > 1), f"I2 {name} mutant {mut}: {f:.3g} of the bar"


@pytest.mark.parametrize("nd", [3, 4])
def test_i3_rejects_the_second_pass_mutants(oracle, nd):
    inp = teeth_inputs(oracle, 4097, 257)
    for k in (5, 33):
        S0 = refine_start(257, k, seed=k)
        for mut in [None] + MUTANTS["I3"]:
            sc, ld, sv = simulate_refine(*inp, S0, nd, mutate=mut)
            d, bar, E, ebar = i3_bars(*inp, sc, ld, sv, nd)
            f, g = frac_of(d, bar), frac_of(E, ebar)
            print(f"I3 nd={nd} k={k}: mutant {mut}: scores {f:.3g}, Gram {g:.3g} of the bar")
            assert (f <= 1 and g <= 1) if mut is None else f > 1, f"I3 k={k} mutant {mut}: {f:.3g} of the bar"


def local_stage_inputs(oracle, N):
    """a row range of the 4097-row matrix that holds SNPs of other blocks: keep = QC's keep and membership, a strict subset"""
    G, mu, sigma, rows = case_inputs(oracle, 4097, N, 1000 * N + 4097)
    r0, r1 = 1203, 2111                                          # 908 rows: no multiple of 32, the range starts off a 32-row unit
    member = np.random.default_rng(3).random(r1 - r0) < 0.7
    keep = (np.isin(np.arange(r0, r1), rows) & member).astype(np.uint8)
    mask = (np.random.default_rng(4).random(N) < 0.4).astype(np.uint8)
    mask[0], mask[-1] = 1, 0
    assert 0 < keep.sum() < np.isin(np.arange(r0, r1), rows).sum()
    return G[r0:r1], mu[r0:r1], sigma[r0:r1], keep, mask, (r0, r1)


@pytest.mark.parametrize("nd", [3, 4])
def test_i4_rejects_zeroed_unmasked_samples(oracle, nd):
    """the oracle's local basis: its features of all samples inside the truth bar, the exact-pass model inside both, and outside with the
    unmasked samples' features zeroed"""
    Gs, mu, sigma, keep, mask, _ = local_stage_inputs(oracle, 257)
    r, b = oracle.scale_shift(mu, sigma, keep)
    U, feats = oracle.eigensnp_local_basis(oracle.standardized_dense(Gs, 257, r, b), mask, 5, 10, 2, 11)
    Wf = (U * keep[:, None]).astype(np.float32)
    m = exact_pass_model(Gs, mu, sigma, Wf, nd)
    bar_model, bar_truth = bounds(m, True)
    held(feats - ref_project(Gs, mu, sigma, Wf)[0], bar_truth, f"I4 nd={nd}: oracle.eigensnp_local_basis against the truth")
    held(m["Y"] - ref_project(Gs, mu, sigma, Wf)[0], bar_truth, f"I4 nd={nd}: the model against the truth")
    mut = m["Y"] * mask[:, None]
    assert frac_of(mut - m["Y"], bar_model) > 1 and frac_of(mut - ref_project(Gs, mu, sigma, Wf)[0], bar_truth) > 1


def test_the_oracle_alone_sits_inside_every_bar(oracle):
    """oracle.eigensnp_global_and_refine (plain f64, LAPACK QR, f64 Omega) through I1, I2 and I3, against the bars of both exact digit
    counts and of GPCA_PREC_F32_MFMA"""
    M, N = 4097, 257
    G, mu, sigma, rows = inp = teeth_inputs(oracle, M, N)
    keep = np.zeros(M, np.uint8); keep[rows] = 1
    A = oracle.standardized_dense(G, N, *oracle.scale_shift(mu, sigma, keep))
    for name, cmax, k, os_, q in (("mixed", 9, 15, 0, 0), ("short_last", 50, 23, 10, 2)):
        W, feat0, R, nb = lay = make_layout(name, M, cmax)
        Wd = dense_basis(W, feat0, R)
        O = oracle.eigensnp_global_and_refine(A, Wd, k, os_, q, 5)
        s0 = O["initial_scores"]
        P = (Wd.T @ A) @ np.linalg.qr(s0)[0]
        sv = np.linalg.norm(s0, axis=0)
        sv_all = np.concatenate([sv, np.zeros(os_)])             # (the trailing values of the oracle's sketch are not returned: the f64 term
        assert np.allclose(np.linalg.svd(P, compute_uv=False), sv, rtol=1e-9)      # only shrinks without them)
        for nd in (3, 4, 0):
            E, bar = i1_bar(G, mu, sigma, rows, np.zeros(len(rows)), Wd, nb, s0, sv, sv_all, k + os_, nd)
            held(E, bar, f"oracle {name} nd={nd}: I1")
            if q == 0:
                Y, Tt, cond = i2_truth(G, mu, sigma, rows, Wd, omega_f32(oracle, R, k, 5), k)
                held(*i2_bar(G, mu, sigma, rows, cmax, s0, Y, Tt, cond, nd), f"oracle {name} nd={nd}: I2")
            svr = np.sqrt(O["eigenvalues"][:k] * (N - 1))
            d, b3, E3, eb3 = i3_bars(G, mu, sigma, rows, O["scores"], O["loadings"][rows], svr, nd)
            held(d, b3, f"oracle {name} nd={nd}: I3 scores"); held(E3, eb3, f"oracle {name} nd={nd}: I3 Gram")


def test_the_bd_restatements_agree_with_the_dense_basis():
    """bd_expand = Wd P and bd_reduce = Wd^T T on every layout (f64 against f64), and a reduce leaves the rows it does not own alone"""
    rng = np.random.default_rng(0)
    for name, M, cmax, l in (("mixed", 4097, 9, 15), ("short_last", 4097, 50, 33), ("one_block", 4097, 64, 32), ("exact_R", 4097, 9, 64), ("small", 33, 7, 5)):
        W, feat0, R, _ = make_layout(name, M, cmax, l)
        Wd = dense_basis(W, feat0, R)
        P = np.zeros((R + 65, l)); P[:R] = rng.standard_normal((R, l))
        T = rng.standard_normal((M, l)).astype(np.float32)
        assert np.max(np.abs(bd_expand(W, feat0, cmax, P) - Wd @ P[:R])) <= 2 * U32 * np.max(np.abs(Wd) @ np.abs(P[:R]))
        Pr = bd_reduce(W, feat0, cmax, T, R, np.full((R + 65, l), 7.0))
        assert np.allclose(Pr[:R], Wd.T @ T.astype(np.float64), rtol=0, atol=1e-12) and np.all(Pr[R:] == 7.0)
        if name == "short_last":
            assert int(feat0.max()) + cmax > R


# ---- the device ----------------------------------------------------------------------------------------------------------------------------
# (layout, M, N, cmax, k, oversample, q)
I1_CASES = [("mixed", 4097, 1025, 9, 15, 0, 2), ("mixed", 4097, 1025, 50, 22, 10, 2), ("mixed", 4097, 257, 50, 64, 0, 0), ("mixed", 4097, 257, 1, 5, 0, 2),
            ("mixed", 4097, 1025, 8, 32, 0, 0), ("short_last", 4097, 257, 9, 33, 0, 2), ("short_last", 4097, 257, 7, 15, 0, 2), ("short_last", 4097, 1025, 64, 54, 10, 0),
            ("one_block", 4097, 257, 64, 32, 0, 2), ("exact_R", 4097, 257, 8, 15, 0, 2), ("exact_R", 4097, 257, 8, 23, 10, 0),
            ("exact_R", 4097, 1025, 9, 64, 0, 2), ("small", 33, 257, 1, 1, 0, 2), ("small", 33, 1025, 7, 5, 10, 0), ("small", 33, 257, 8, 1, 0, 0)]
# (layout, M, N, cmax, l): q = 0, oversample = 0, R >= 2 l
I2_CASES = [("mixed", 4097, 257, 9, 15), ("mixed", 4097, 257, 50, 64), ("mixed", 4097, 1025, 8, 1), ("short_last", 4097, 1025, 7, 15),
            ("short_last", 4097, 257, 64, 33), ("one_block", 4097, 257, 64, 32), ("small", 33, 257, 7, 5), ("small", 33, 257, 1, 1)]


def condensed_call(e, G, mu, sigma, rows, lay, k, os_, q):
    e.upload_genotypes_i8(G)
    ulps = device_stats(e, mu, sigma, rows)
    e.set_condensed_basis(lay[0], lay[1], lay[2])
    e.rsvd_condensed(k, os_, q, seed=5)
    sv = np.sqrt(e.eigenvalues() * (G.shape[1] - 1))
    return ulps, e.scores(f64=True), sv, e.singular_values()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name,M,N,cmax,k,os_,q", I1_CASES)
def test_i1_forward_product(oracle, mode, name, M, N, cmax, k, os_, q):
    G, mu, sigma, rows = case_inputs(oracle, M, N, 1000 * N + M)
    lay = make_layout(name, M, cmax, k + os_)
    assert k + os_ <= min(lay[2], len(rows), N)
    with open_engine(mode) as e:
        ulps, S, sv, sv_all = condensed_call(e, G, mu, sigma, rows, lay, k, os_, q)
    assert np.allclose(sv_all[:k], sv, rtol=1e-12)
    E, bar = i1_bar(G, mu, sigma, rows, ulps, dense_basis(*lay[:3]), lay[3], S, sv, sv_all, k + os_, MODES[mode][3])
    held(E, bar, f"I1 {mode} {name} M={M} N={N} cmax={cmax} k={k}+{os_} q={q} R={lay[2]}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name,M,N,cmax,l", I2_CASES)
def test_i2_backward_product(oracle, mode, name, M, N, cmax, l):
    G, mu, sigma, rows = case_inputs(oracle, M, N, 1000 * N + M)
    lay = make_layout(name, M, cmax, l)
    Y, Tt, cond = i2_truth(G, mu, sigma, rows, dense_basis(*lay[:3]), omega_f32(oracle, lay[2], l, 5), l)      # (both conditions: before the launch)
    with open_engine(mode) as e:
        _, S, _, _ = condensed_call(e, G, mu, sigma, rows, lay, l, 0, 0)
    held(*i2_bar(G, mu, sigma, rows, cmax, S, Y, Tt, cond, MODES[mode][3]), f"I2 {mode} {name} M={M} N={N} cmax={cmax} l={l} R={lay[2]}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("N", [257, 1025])
def test_i3_refine_scores_side(oracle, mode, N):
    M, nd = 4097, MODES[mode][3]
    G, mu, sigma, rows = case_inputs(oracle, M, N, 1000 * N + M)
    with open_engine(mode) as e:
        e.upload_genotypes_i8(G)
        device_stats(e, mu, sigma, rows)
        e.set_standardization(mu, sigma, np.isin(np.arange(M), rows).astype(np.uint8))      # (the CPU's sigma, as test_refine of the K1 module)
        for k in (1, 5, 33, 64):
            e.refine(refine_start(N, k, seed=N + k))
            S, ld, sv = e.scores(f64=True), e.loadings(), np.sqrt(e.eigenvalues() * (N - 1))
            d, bar, E, ebar = i3_bars(G, mu, sigma, rows, S, ld, sv, nd)
            held(d, bar, f"I3 {mode} N={N} k={k}: scores = A^T loadings")
            held(E, ebar, f"I3 {mode} N={N} k={k}: scores^T scores = diag(sv^2)")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", EXACT)
@pytest.mark.parametrize("N", [257, 1025])
def test_i4_local_stage(oracle, mode, N):
    nd = MODES[mode][3]
    G, _, _, _ = case_inputs(oracle, 4097, N, 1000 * N + 4097)
    Gs, mu, sigma, keep, mask, (r0, r1) = local_stage_inputs(oracle, N)
    rows = np.flatnonzero(keep)
    with open_engine(mode) as e, open_engine(mode) as sub:
        e.upload_genotypes_i8(G)
        sub.copy_rows_from(e, r0, r1 - r0)
        sub.set_standardization(mu, sigma, keep)
        sub.set_sample_mask(mask)
        for k, os_ in ((5, 10), (33, 0)):
            sub.rsvd(k, os_, 2, seed=11)
            sc, sv, ld, feats = sub.scores(f64=True), sub.singular_values(), sub.loadings(), sub.transform()
            assert np.array_equal(sub.pca_snp_rows(), rows) and np.all(sc[mask == 0] == 0.0)
            truth = k1_truth(Gs, mu, sigma, rows, sc, sv, mask)
            check(ld, truth, k1_bar(Gs, mu, sigma, rows, sc, sv, k + os_, nd, truth, mask), f"I4 {mode} N={N} k={k}+{os_}: the masked fit's loadings")
            Wf = np.zeros((r1 - r0, k), np.float32)
            Wf[rows] = ld
            check_against_bars(feats, Gs, mu, sigma, Wf, nd, True, f"I4 {mode} N={N} k={k}+{os_}: features of all samples")
            assert np.any(feats[mask == 0] != 0)


@pytest.mark.gpu
def test_a_condensed_call_repeats_bit_for_bit(oracle):
    """cmax = 50, a short block before larger ones and last: every block writes its own features only, the same bits every time"""
    G, mu, sigma, rows = case_inputs(oracle, 4097, 257, 1000 * 257 + 4097)
    for name in ("mixed", "short_last"):
        lay = make_layout(name, 4097, 50)
        with open_engine("int8") as e:
            _, S, sv, _ = condensed_call(e, G, mu, sigma, rows, lay, 22, 10, 2)
            for _ in range(3):
                e.rsvd_condensed(22, 10, 2, seed=5)
                assert np.array_equal(e.scores(f64=True), S) and np.array_equal(np.sqrt(e.eigenvalues() * 256), sv)
