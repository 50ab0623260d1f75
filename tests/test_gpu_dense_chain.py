"""The small dense chain between the GEMM sweeps -- CholeskyQR (stage_orth: k_gram_mfma / k_gram_any, k_sum_partials, k_chol_inv<32>,
k_chol_inv<64>, k_chol_inv_fold32, k_chol_inv_any, k_apply_right, k_apply_right_tail, k_apply_right_any, k_finish_q and the finishq fold)
and the tail of a call (the eigen step as the product calls it, k_scores, k_scores_sign, k_col_sign, k_scale_cols, k_rightmul_any,
k_rightmul_mfma with the sign) -- held to bars derived from their arithmetic, on a caller's own input through the two test hooks
gpca_device_orth and gpca_device_tail (include/gpca.h), which run the product's own stage functions.  Style of test_gpu_k1_pass.py and
test_gpu_eigensnp_stages.py.  Every reference is numpy.longdouble arithmetic on the uploaded input and the returned output; the device is
never compared with another device path (the one exception is asked for: equal bits of Q across precisions and storages).

NOTATION.  u = 2^-53, u32 = 2^-24, Y [N][l] the uploaded sketch, Q [N][l] what comes back, L = l padded to 32 / 64 / 128,
g = N l u + l (l + 1) u (the Gram's N-term sums over l columns and the factorisation's l (l + 1) / 2 updates, twice), kappa = cond(Y).
The carrier matrix is 130 SNP rows x N with mu = 0, sigma = 1: the chain never reads a genotype.

(a) ORTHONORMALISATION.  Three backward-error statements, none of which depends on how the columns of Q could legitimately differ:
  orthonormality   |Q^T Q - I|_F <= 6 g for rounds = 2: the CholeskyQR2 bound of Yamamoto, Nakatsukasa, Yanagisawa and Fukaya (2015), whose
                   precondition 8 kappa sqrt(g) <= 1 is asserted on the CPU before anything is launched; rounds = 1: kappa^2 6 g.
  residual         |Y - Q (Q^T Y)|_F <= 5 l^2 u |Y|_2 (Q = Y R^-1: l-term sums against an l x l triangle, 5 from the same paper's lemma)
  triangularity    Q^T Y is upper triangular with a positive diagonal, its strictly lower part (Frobenius) under the residual bar.
  With rounds = 1 the same two statements are made about Q^+ Y, Q^+ = (Q^T Q)^-1 Q^T in longdouble: Q^T Y = (I + d) R carries the one
  round's own d = Q^T Q - I (1.4e-11 .. 1.6e-9 at kappa = 1e3 .. 1e4) times |Y|, which is not an error of the kernels; Q^+ = Q^T where d = 0.
  s = Q^T 1    against the longdouble column sums of the device's own Q: u (tail_num_parts + 64) sum_n |Q_nj| (64 rows per workgroup of
               the last right-multiplication, then one partial per workgroup, folded in any order).
  Y = U diag(logspace(0, -log10 kappa)) V^T with kappa = 1e4, or 1e3 where the precondition does not allow 1e4 (at least 1e3, so that one
  round where two were asked leaves the bar: the tooth ``one_round``).  Shapes: the smallest that reach each branch of plan_math.h and the
  launchers -- l = 1, 2, 31, 32, 33, 63, 64, 65, 100, 127, 128 (k_chol_inv<32> against _fold32, <64>, _any with k_gram_any and
  k_apply_right_any, n < L identity padding at every L); N = l from 32 on; N = 33, 255, 256, 257, 1000 (the last Gram block partial,
  gram_rows_per_block at its floor); 8193 and 16 400 (more Gram parts); 33 000 (tail_num_parts > kFinishQFoldMax: launch_finish_q +
  _prescaled in place of the finishq fold); 262 145 once at l = 20 (more than 64 Gram parts: k_sum_partials + k_chol_inv<32>).
  Contracts of the Cholesky, exact: a duplicated column, a zero column and the last of l = N centred columns come back as exactly zero
  columns of Q with the flag 0 and the bars holding on the rest; a column whose pivot ratio is 1e-10 stays (kCholRankTol = 1e-13); one
  Inf / one NaN in column j gives pivot_flag = j + 1 while the hook returns GPCA_OK; a sample mask leaves exactly zero rows; the f64
  part does not depend on precision or storage: equal bits of Q on GPCA_PREC_F32_MFMA and on 2-bit rows.
(b) THE TAIL.  Q is the caller's, so the right-multiplication and the sign rule are tested as what they are.
  scores = Q Z0    the rows e_0 .. e_{l-1} are planted in Q, so Z0 (with its sign) comes back bit for bit through the scores (products by 1
                   and sums with +0 are exact); every other score against the longdouble product with that Z0: u (L + 1) sum_j |Q_nj Z0_jc|
                   (a chain of L fmas); f32 scores = float32(f64 scores) bit for bit.
  sign             two rows that are exact negatives of each other hold the largest magnitude of every column (at rows (0, 1), (255, 256): a
                   chunk boundary, (12 287, 12 288): chunk 48 returns to workgroup 0 under kScoreParts = 48, (5, N - 1); L = 128:
                   (1023, 1024) and (4095, 4096), the strides of k_col_sign), either one first: the LOWER row is positive in every column;
                   the loadings carry the same sign (zmode 1, selection rows in B: loadings = float32(Z0) bit for bit); an all-zero column
                   of scores keeps sign +1 (seen as +0.0: a flipped column would hold -0.0).
  eigen step       w := sv^2 against numpy.linalg.eigvalsh of the longdouble Gram: |u R (|X|^T |X|)|_F (R-term sums, R = 130 rows of B or N
                   rows of Q) + 1e-12 w_0 (what test_device_eigensolver_against_the_host_pin_and_lapack holds the solver to; not re-derived
                   here) + 4 u w (sv is a rounded square root: 1 ulp = 2 u, squared); max |C V_k - V_k w| <= 1e-11 w_0 with V_k read from
                   Z0; |sv^2 - eig denom| <= ((1 + 2 u)^2 (1 + 2 u) - 1) sv^2 (sv within 1 ulp of sqrt(w), eig denom = w within 2 u);
                   zmode 0 with selection rows in B: |loadings - Z0 / sv^2| <= (3 u + u32) |Z0 / sv^2| (Z1 comes back as f32: one store
                   rounding); a zero column of B gives sv = 0 and an exactly zero column of loadings; nothing anywhere is Inf or NaN.
                   l = 1, 31, 32, 33, 64 with k = l and k < l, l = 100 (QL path) with k = 90, both zmodes, M = 130 and 130 with 40 rows
                   dropped by keep (the gather; the dropped rows of B hold NaN and are never read).
(c) TEETH (CPU, unmarked).  ``sim_orth`` / ``sim_tail`` run the device recipe in numpy: the Gram in gram_rows_per_block blocks,
  right-looking Cholesky with the kCholRankTol rule, R^-1 by back substitution, the apply, the chunked sign fold and the strided one of
  k_col_sign.  The unmutated simulator and a Householder QR sit inside every bar on the device tests' own inputs (N <= 1000); each mutant
  of ORTH_MUTANTS / TAIL_MUTANTS leaves its bar or fails its exact check.

NOT REACHED, AND WHY.  The f32 blocked basis dQ and the digit planes of Q (the K1 tests reach them through the loadings).  The cap flag
of the eigen kernels cannot be forced honestly on the device (tests/test_eig_result_audit.py pins the verdict on the CPU).  A second
device.  Loadings of non-selection rows in zmode 0 (Z1 is only known to f32 from outside; zmode 1 checks every row of k_rightmul_mfma
and k_rightmul_any).  The sign of an all-zero column is only visible as the sign of zero.

Measured on the CPU (the teeth), the largest fraction of each bar: Householder QR orthonormality 0.0033, residual 0.33, triangularity
0.026; the simulator 0.0079, 0.13, 0.011, s 0.029, one round 0.0021 / 0.028 / 0.0020; its tail scores 0.29, w 0.0013, eig denom 0.43, Z1 and
loadings 0.997 (an f32 store rounds by up to u32: this term is the bar).  The weakest mutant is
``one_round`` (N = 1000, l = 128: 23 x its bar), every other mutant is more than 1e10 x outside or fails an exact check.
Measured on one MI355X, the largest fraction of each bar over every case (records, not thresholds; each test prints its own with -s):
    orthonormalisation, two rounds   orthonormality 0.0065, residual 0.45 (l = 2 at N = 256; 0.0019 from N = 8193 on), triangularity 0.0050, s 0.030
    orthonormalisation, one round    orthonormality 0.00077 of kappa^2 6 g, residual 0.030 and triangularity 0.0020 (of Q^+ Y), s 0.013
    scores and sign cases            scores 0.36, w 0.0010, residual 5.8e-05, eig denom 0.42, Z1 0.993 and loadings 0.995 (the f32 store)
    eigen step cases                 scores 0.26, w 0.010, residual 0.00090, eig denom 0.42, Z1 0.998 and loadings 0.99 (the f32 store)
    every exact check held; the whole module takes 10 s."""
import ctypes as C

import numpy as np
import pytest

from genomic_pca_amd import _lib

LD = np.longdouble
U, U32 = 2.0 ** -53, 2.0 ** -24
CHOL_TOL = 1e-13                       # kCholRankTol (kernels.hip)
EIG, EIG_RES = 1e-12, 1e-11            # test_device_eigensolver_against_the_host_pin_and_lapack (test_gpu_parity.py)
M_CARRIER = 130
MODES = {"int8": (_lib.PREC_I8_EXACT, _lib.STORE_INT8), "2bit": (_lib.PREC_I8_EXACT, _lib.STORE_2BIT), "f32": (_lib.PREC_F32_MFMA, _lib.STORE_INT8)}


# ---- plan_math.h, restated (tests/cpp/plan_audit.cpp walks the header itself) ------------------------------------------------------------
def padded(l):
    return 32 if l <= 32 else (64 if l <= 64 else 128)


def gram_rows_per_block(rows):
    if rows <= 262144:
        parts = min(max(rows // 256, 32), 64)
        q = -(-rows // parts)
        return 32 if q < 32 else (q + 31) // 32 * 32
    r = (-(-rows // 1024) + 31) // 32 * 32
    return min(max(r, 32), 2048)


def gram_num_parts(rows):
    return -(-rows // gram_rows_per_block(rows))


def tail_num_parts(N):
    return -(-(-(-N // 256) * 256) // 64)          # rows padded to kSamplePad = 256, kTailRows = 64 per workgroup


def scores_num_parts(rows):
    return min(max(-(-rows // 256), 1), 48)


# ---- longdouble helpers ------------------------------------------------------------------------------------------------------------------
def ld(a):
    return np.asarray(a).astype(LD)


def mm_tn(A, B):
    """A^T B in longdouble (einsum: numpy has no BLAS for this type, and its matmul is five times slower)"""
    return np.einsum("ni,nj->ij", ld(A), ld(B))


def mm(A, B):
    return np.einsum("nk,kj->nj", ld(A), ld(B))


def fro(a):
    return float(np.sqrt(np.sum(ld(a) ** 2)))


def frac(value, bar):
    """value / bar; a non-finite value, or a positive one over a zero bar, is infinitely far out"""
    value, bar = float(value), float(bar)
    if not np.isfinite(value) or not np.isfinite(bar):
        return np.inf
    return value / bar if bar > 0 else (np.inf if value > 0 else 0.0)


def frac_elems(d, bar):
    d, bar = np.abs(np.asarray(d, np.float64)), np.asarray(bar, np.float64)
    if not (np.all(np.isfinite(d)) and np.all(np.isfinite(bar))):
        return np.inf
    return float(np.max(np.where(bar > 0, d / np.where(bar > 0, bar, 1), np.where(d > 0, np.inf, 0)), initial=0))


# ---- (a) inputs and checks ---------------------------------------------------------------------------------------------------------------
def g_of(N, l):
    return (N * l + l * (l + 1)) * U


def kappa_for(N, l):
    """1e4 inside the CholeskyQR2 precondition 8 kappa sqrt(g) <= 1, else 1e3 (never less: one round must leave the two-round bar)"""
    if l == 1:
        return 1.0
    return 1e4 if 8e4 * np.sqrt(g_of(N, l)) <= 1 else 1e3


def planted(N, l, kappa, seed):
    """Y = U diag(logspace(0, -log10 kappa)) V^T, U [N][l] and V [l][l] with orthonormal columns"""
    rng = np.random.default_rng(seed)
    Uo, _ = np.linalg.qr(rng.standard_normal((N, l)))
    V, _ = np.linalg.qr(rng.standard_normal((l, l)))
    return np.ascontiguousarray((Uo * np.logspace(0, -np.log10(kappa), l)) @ V.T)


def orth_input(N, l, seed=None):
    return planted(N, l, kappa_for(N, l), 7919 * N + l if seed is None else seed)


def precondition(Y):
    """cond(Y), after asserting 8 cond(Y) sqrt(g) <= 1"""
    N, l = Y.shape
    sv = np.linalg.svd(Y, compute_uv=False)
    kappa = float(sv[0] / sv[-1])
    assert 8 * kappa * np.sqrt(g_of(N, l)) <= 1, f"CholeskyQR2 precondition broken at {N} x {l}: cond = {kappa:.3g}"
    return kappa


def orth_fractions(Y, Q, rounds, kappa=None, count_rows=None):
    """{name: value / bar} of the three backward-error statements for Q against Y (full column rank)"""
    N, l = Y.shape
    g = g_of(count_rows or N, l)
    if kappa is None:
        sv = np.linalg.svd(Y, compute_uv=False)
        kappa = float(sv[0] / sv[-1])
    if not np.all(np.isfinite(Q)):
        return {"orthonormality": np.inf, "residual": np.inf, "triangularity": np.inf, "diagonal": np.inf}
    QtQ = mm_tn(Q, Q)
    out = {"orthonormality": frac(fro(QtQ - np.eye(l, dtype=LD)), 6 * g * (1.0 if rounds == 2 else kappa ** 2))}
    R = mm_tn(Q, Y)
    if rounds == 1:                      # Q^+ Y: see the module docstring
        R = ld(np.linalg.solve(QtQ.astype(np.float64), R.astype(np.float64)))
        R = R + ld(np.linalg.solve(QtQ.astype(np.float64), (mm_tn(Q, Y) - QtQ @ R).astype(np.float64)))      # one step of refinement in longdouble
    bar = 5 * l * l * U * float(np.linalg.norm(Y, 2))
    out["residual"] = frac(fro(ld(Y) - mm(Q, R)), bar)
    out["triangularity"] = frac(fro(np.tril(R, -1)), bar)
    out["diagonal"] = 0.0 if np.all(np.diag(R) > 0) else np.inf
    return out


def s_fraction(Q, s):
    N = Q.shape[0]
    ref = np.sum(ld(Q), axis=0)
    bar = U * (tail_num_parts(N) + 64) * np.sum(np.abs(Q), axis=0)
    return frac_elems((ld(s) - ref).astype(np.float64), bar)


def report(what, fr):
    print(f"{what}: " + "  ".join(f"{k} {v:.3g}" for k, v in fr.items()))
    return fr


def inside(fr):
    return all(v <= 1.0 for v in fr.values())


def dependent_inputs(N, l, kind, seed=3):
    """(Y, dropped column, kept columns): a well-conditioned sketch with one dependent column"""
    rng = np.random.default_rng(seed + N + l)
    if kind == "centred":                # l = N centred columns: rank N - 1, the last column is the one that has nothing left
        assert N == l
        H = rng.standard_normal((N, N - 1))
        H, _ = np.linalg.qr(H - H.mean(axis=0, keepdims=True))          # an orthonormal basis of the centred vectors
        Y = np.empty((N, l))
        Y[:, :-1] = H @ planted(N - 1, N - 1, 10.0, seed + N)           # N - 1 independent centred columns of condition 10 ...
        Y[:, -1] = -Y[:, :-1].sum(axis=1)                               # ... and the one that completes them to zero row sums
        Y -= Y.mean(axis=0, keepdims=True)
        j = l - 1
    else:
        Y = planted(N, l, 10.0, seed + N + l)
        j = (2 * l) // 3
        Y[:, j] = Y[:, 1] if kind == "duplicate" else 0.0
    return np.ascontiguousarray(Y), j, np.array([c for c in range(l) if c != j])


def small_pivot_input(N, l, ratio=1e-10, seed=5):
    """column j = u_i + sqrt(ratio) u_j for orthonormal u: what is left of its squared norm after the elimination is `ratio` of it"""
    rng = np.random.default_rng(seed + N + l)
    Uo, _ = np.linalg.qr(rng.standard_normal((N, l)))
    R = np.eye(l)
    i, j = 1, (2 * l) // 3
    R[i, j], R[j, j] = 1.0, np.sqrt(ratio)
    return np.ascontiguousarray(Uo @ R), j


# ---- (b) inputs and checks ---------------------------------------------------------------------------------------------------------------
class TailCase:
    """Q [N][l] f64 with the rows e_j planted at ``ident`` (None where column j of Q is all zero) and an optional pair of exact negatives
    that holds the largest magnitude of every column; B [M][l] f32 with the rows e_j at ``sel`` (None where column j of B is all zero) and
    a planted spectrum in the other kept rows; the dropped rows of B hold NaN."""

    def __init__(self, N, l, k, zmode, pair=None, neg_first=False, keep=None, zero_col=None, seed=0):
        rng = np.random.default_rng(1000 * l + 10 * k + zmode + seed)
        self.N, self.l, self.k, self.zmode, self.pair, self.zero_col = N, l, k, zmode, pair, zero_col
        self.keep = np.ones(M_CARRIER, np.uint8) if keep is None else np.asarray(keep, np.uint8)
        rows = np.flatnonzero(self.keep)
        self.rows = rows
        assert l <= min(len(rows), N) and 1 <= k <= l
        # Q: a planted spectrum (zmode 1 reads its Gram), the identity rows away from the pair rows and the chunk edges
        spec = np.logspace(0, -2, l) if l > 1 else np.ones(1)
        Q = rng.standard_normal((N, l)) * spec
        taken = set(pair or ())
        free = [r for r in range(7, N - 1) if r not in taken and (r % 256) not in (0, 255)]
        step = max(1, len(free) // (l + 1))
        self.ident = [free[(j + 1) * step - 1] for j in range(l)]
        for j, r in enumerate(self.ident):
            Q[r] = 0.0
            Q[r, j] = 1.0
        if pair is not None:
            p = 1e5 * rng.standard_normal(l)
            a, b = pair
            Q[a], Q[b] = (-p, p) if neg_first else (p, -p)
        # B: selection rows first, the planted spectrum in the other kept rows
        B = np.zeros((M_CARRIER, l), np.float32)
        self.sel = [int(rows[j]) for j in range(l)]
        for j, r in enumerate(self.sel):
            B[r, j] = 1.0
        rest = rows[l:]
        if len(rest):
            B[rest] = (rng.standard_normal((len(rest), l)) * np.logspace(1.5, 0, l)).astype(np.float32)
        if zero_col is not None:
            B[:, zero_col] = 0.0
            self.sel[zero_col] = None
            if zmode == 1:               # zmode 1 reads the Gram of Q: the zero column is Q's, and no identity row can sit in it
                Q[:, zero_col] = 0.0
                self.ident[zero_col] = None
        B[self.keep == 0] = np.nan
        self.Q, self.B = np.ascontiguousarray(Q), np.ascontiguousarray(B)
        self.denom = float(N - 1)


def tail_fractions(case, out, eigen=True):
    """{name: value / bar, or 0 / inf for an exact check} for the results `out` of one tail on `case`; eigen = False leaves out the two
    checks that need the longdouble Gram (the sign cases at 12 588 samples: the eigen step has its own cases)"""
    N, l, k, zmode, Q = case.N, case.l, case.k, case.zmode, case.Q
    L = padded(l)
    S64, S32, sv, eig, load = out["scores64"], out["scores32"], out["sv"], out["eig"], out["loadings"]
    fr = {}
    fr["finite"] = 0.0 if all(np.all(np.isfinite(out[x])) for x in ("scores64", "scores32", "sv", "eig", "loadings")) else np.inf
    if fr["finite"]:
        return fr
    fr["f32 scores"] = 0.0 if np.array_equal(S32.view(np.uint32), S64.astype(np.float32).view(np.uint32)) else np.inf
    # Z0 with its sign, bit for bit through the identity rows; a row that could not be planted (zero column of Q) is e_j's own: V holds
    # +-e_j in the column of the zero eigenvalue and zero elsewhere in that row, and no score depends on it
    Z0 = np.zeros((l, k))
    for j, r in enumerate(case.ident):
        if r is not None:
            Z0[j] = S64[r]
    ref = mm(Q, Z0)
    fr["scores"] = frac_elems((ld(S64) - ref).astype(np.float64), U * (L + 1) * (np.abs(Q) @ np.abs(Z0)))
    # the sign rule: the first row of maximal |score| is positive; an all-zero column holds +0.0
    a = np.abs(S64)
    first = np.argmax(a, axis=0)
    top = S64[first, np.arange(k)]
    zero = a.max(axis=0) == 0
    fr["sign"] = 0.0 if np.all(top[~zero] > 0) and not np.any(np.signbit(S64[:, zero])) else np.inf
    if case.pair is not None:            # zmode 0: the pair holds every column's maximum; zmode 1 (Z0 = the eigenvectors of Q^T Q, which the
        lo, hi = min(case.pair), max(case.pair)      # pair itself dominates): the leading column's, all other columns are orthogonal to it
        tie = (a[lo] == a.max(axis=0)) & ~zero
        assert np.all(tie | zero) if zmode == 0 else tie[0], "the planted pair must hold the maximum of every column (zmode 1: of the first)"
        fr["pair"] = 0.0 if np.array_equal(S64[lo], -S64[hi]) and np.all(S64[lo, tie] > 0) and np.all(first[tie] == lo) else np.inf
    # the eigen step
    wdev = ld(sv) ** 2
    pos = sv[:k] > 0
    if eigen:
        X = ld(case.B[case.rows]) if zmode == 0 else ld(Q)
        Rn = M_CARRIER if zmode == 0 else N
        Cm = mm_tn(X, X)
        wref = np.linalg.eigvalsh(Cm.astype(np.float64))[::-1]
        w0 = max(abs(wref[0]), 1e-300)
        gram_bar = U * Rn * fro(np.abs(X).T @ np.abs(X))
        fr["w"] = frac_elems((wdev - ld(wref)).astype(np.float64), gram_bar + EIG * w0 + 4 * U * wdev.astype(np.float64))
        Vk = ld(Z0) if zmode == 1 else ld(Z0)[:, pos] / ld(sv[:k][pos])
        wk = wdev[:k] if zmode == 1 else wdev[:k][pos]
        live = [j for j in range(l) if case.ident[j] is not None]      # (a zero column of Q: its row of C is zero, and so is the residual's)
        fr["residual"] = frac(np.max(np.abs((Cm @ Vk - Vk * wk)[live]), initial=0), EIG_RES * w0)
    if case.zero_col is not None:        # an exactly zero column of the factor: the last singular value is exactly zero
        fr["sv = 0"] = 0.0 if sv[-1] == 0.0 else np.inf
    fr["descending"] = 0.0 if np.all(np.diff(sv) <= 0) and np.all(sv >= 0) else np.inf
    rel = float((LD(1) + 2 * LD(U)) ** 3 - 1)
    fr["eig denom"] = frac_elems((wdev[:k] - ld(eig) * LD(case.denom)).astype(np.float64), rel * wdev[:k].astype(np.float64))
    # the loadings
    Lsel = np.array([load[np.searchsorted(case.rows, r)] if r is not None else np.zeros(k, np.float32) for r in case.sel])
    have = np.array([r is not None for r in case.sel])
    if zmode == 1:
        fr["loadings sign"] = 0.0 if np.array_equal(Lsel[have], Z0[have].astype(np.float32)) else np.inf      # (values: a sum may turn -0 into +0)
        Bk = case.B[case.rows]
        fr["loadings"] = frac_elems((ld(load) - mm(Bk, Z0)).astype(np.float64),
                                    (U32 + U * (L + 1)) * (np.abs(Bk).astype(np.float64) @ np.abs(Z0)))
    else:
        Z1 = np.zeros((l, k), LD)
        Z1[:, pos] = ld(Z0)[:, pos] / wdev[:k][pos]
        fr["Z1"] = frac_elems((ld(Lsel) - Z1).astype(np.float64)[have], ((3 * U + U32) * np.abs(Z1)).astype(np.float64)[have])
        fr["loadings where sv = 0"] = 0.0 if np.all(load[:, ~pos] == 0) else np.inf
    return fr


# ---- the device ----------------------------------------------------------------------------------------------------------------------------
def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def open_carrier(gpca, N, mode="int8", keep=None):
    prec, store = MODES[mode]
    e = gpca.GpcaEngine(precision=prec, storage=store)
    G = ((np.arange(M_CARRIER)[:, None] + 2 * np.arange(N)[None, :]) % 3).astype(np.int8)
    e.upload_genotypes_i8(G)
    e.set_standardization(np.zeros(M_CARRIER, np.float32), np.ones(M_CARRIER, np.float32), keep)
    return e


@pytest.fixture(scope="module")
def carriers(gpca):
    """one handle per (N, mode, keep), reused by every case of the module"""
    held = {}

    def get(N, mode="int8", keep=None):
        key = (N, mode, None if keep is None else bytes(np.asarray(keep, np.uint8)))
        if key not in held:
            held[key] = open_carrier(gpca, N, mode, keep)
        return held[key]
    yield get
    for e in held.values():
        e.close()


def dev_orth(e, Y, rounds=2, want_rc=0):
    lib = _lib.load()
    Y = np.ascontiguousarray(Y, np.float64)
    N, l = Y.shape
    Q, s, flag = np.full((N, l), np.nan), np.full(l, np.nan), C.c_int32(-1)
    rc = lib.gpca_device_orth(e._h, _vp(Y), l, rounds, _vp(Q), _vp(s), C.byref(flag))
    assert rc == want_rc, (rc, lib.gpca_last_error(e._h))
    return Q, s, flag.value


def dev_tail(e, case):
    lib = _lib.load()
    N, l, k = case.N, case.l, case.k
    rc = lib.gpca_device_tail(e._h, _vp(case.Q), _vp(case.B), l, k, case.zmode)
    assert rc == 0, (rc, lib.gpca_last_error(e._h))
    out = {"scores64": np.empty((N, k)), "scores32": np.empty((N, k), np.float32), "sv": np.empty(l), "eig": np.empty(k),
           "loadings": np.empty((len(case.rows), k), np.float32)}
    assert lib.gpca_get_scores_f64(e._h, _vp(out["scores64"])) == 0 and lib.gpca_get_scores(e._h, _vp(out["scores32"])) == 0
    assert lib.gpca_get_singular_values(e._h, _vp(out["sv"])) == 0 and lib.gpca_get_eigenvalues(e._h, _vp(out["eig"])) == 0
    assert lib.gpca_get_loadings(e._h, _vp(out["loadings"])) == 0
    return out


ALL_L = [1, 2, 31, 32, 33, 63, 64, 65, 100, 127, 128]
ORTH_SHAPES = {33: [l for l in ALL_L if l <= 33], 255: ALL_L, 256: ALL_L, 257: ALL_L, 1000: ALL_L,
               32: [32], 63: [63], 64: [64], 65: [65], 100: [100], 127: [127], 128: [128],      # N = l (33 x 33 rides with N = 33)
               8193: [31, 33], 16400: [31, 33], 33000: [32, 64]}
ROUND1_L = (2, 32, 33, 100)              # one round: one l per kernel family


def run_orth_case(e, N, l, rounds):
    Y = orth_input(N, l)
    kappa = precondition(Y)
    Q, s, flag = dev_orth(e, Y, rounds)
    assert flag == 0
    fr = orth_fractions(Y, Q, rounds, kappa)
    fr["s"] = s_fraction(Q, s)
    report(f"orth N={N} l={l} rounds={rounds} cond={kappa:.3g}", fr)
    assert inside(fr), (N, l, rounds, fr)
    return fr


@pytest.mark.gpu
@pytest.mark.parametrize("N", sorted(ORTH_SHAPES))
def test_orthonormalisation_against_longdouble(gpca, N):
    worst = {}
    with open_carrier(gpca, N) as e:
        for l in ORTH_SHAPES[N]:
            for rounds in ((2, 1) if l in ROUND1_L else (2,)):
                for name, v in run_orth_case(e, N, l, rounds).items():
                    worst[(name, rounds)] = max(worst.get((name, rounds), 0.0), v)
    print(f"orth N={N}: worst fractions " + "  ".join(f"{n}/r{r} {v:.3g}" for (n, r), v in sorted(worst.items())))


@pytest.mark.gpu
def test_orthonormalisation_beyond_64_gram_parts(gpca):
    """262 145 rows make 911 Gram parts: at L = 32 k_chol_inv_fold32 gives way to k_sum_partials + k_chol_inv<32>"""
    N, l = 262145, 20
    assert gram_num_parts(N) > 64 and kappa_for(N, l) == 1e3
    with open_carrier(gpca, N) as e:
        run_orth_case(e, N, l, 2)


@pytest.mark.gpu
def test_sample_mask_rows_are_zero_and_the_rest_holds_the_bars(gpca):
    N = 1000
    mask = (np.arange(N) % 3 != 1).astype(np.uint8)
    with open_carrier(gpca, N) as e:
        e.set_sample_mask(mask)
        for l in (31, 64, 100):
            Y = orth_input(N, l)
            Ym = Y[mask != 0]
            kappa = precondition(Ym)
            Q, s, flag = dev_orth(e, Y, 2)
            assert flag == 0 and np.all(Q[mask == 0] == 0.0)
            fr = orth_fractions(Ym, Q[mask != 0], 2, kappa, count_rows=N)
            fr["s"] = s_fraction(Q, s)
            report(f"masked orth N={N} l={l}", fr)
            assert inside(fr), (l, fr)
        e.set_sample_mask(None)


@pytest.mark.gpu
def test_q_has_the_same_bits_on_every_precision_and_storage(gpca):
    N = 1000
    got = {}
    for mode in ("int8", "f32", "2bit"):
        with open_carrier(gpca, N, mode) as e:
            for l in (31, 33, 64):
                Q, s, flag = dev_orth(e, orth_input(N, l), 2)
                assert flag == 0
                fr = {"s": s_fraction(Q, s)}
                report(f"orth on {mode} N={N} l={l}", fr)
                assert inside(fr)
                got[(mode, l)] = Q
    for mode in ("f32", "2bit"):
        for l in (31, 33, 64):
            assert np.array_equal(got[(mode, l)].view(np.uint64), got[("int8", l)].view(np.uint64)), (mode, l)


CONTRACT_L = (30, 60, 100)               # L = 32, 64, 128


@pytest.mark.gpu
def test_cholesky_rank_contracts(gpca):
    N = 257
    with open_carrier(gpca, N) as e:
        for l in CONTRACT_L:
            for kind in ("duplicate", "zero"):
                Y, j, rest = dependent_inputs(N, l, kind)
                Q, _, flag = dev_orth(e, Y, 2)
                assert flag == 0 and np.all(Q[:, j] == 0.0), (l, kind)
                fr = report(f"{kind} column N={N} l={l}", orth_fractions(Y[:, rest], Q[:, rest], 2, precondition(Y[:, rest])))
                assert inside(fr), (l, kind, fr)
            Y, j = small_pivot_input(N, l)
            Q, _, flag = dev_orth(e, Y, 2)
            assert flag == 0 and np.all(np.isfinite(Q)) and np.linalg.norm(Q[:, j]) > 0.5, (l, "a pivot ratio of 1e-10 is not a dependent column")
    for l in (32, 64, 128):
        with open_carrier(gpca, l) as e:
            Y, j, rest = dependent_inputs(l, l, "centred")
            Q, _, flag = dev_orth(e, Y, 2)
            assert flag == 0 and np.all(Q[:, j] == 0.0), l
            fr = report(f"centred columns N=l={l}", orth_fractions(Y[:, rest], Q[:, rest], 2, precondition(Y[:, rest])))
            assert inside(fr), (l, fr)


@pytest.mark.gpu
def test_non_finite_sketch_sets_the_pivot_flag(gpca):
    """Only the orth hook: it runs no GEMM and no eigen kernel.  The flag is data; the hook returns GPCA_OK."""
    N = 257
    with open_carrier(gpca, N) as e:
        for l in CONTRACT_L:
            for bad in (np.inf, np.nan):
                for j in (0, l // 2, l - 1):
                    Y = orth_input(N, l)
                    Y[N // 2, j] = bad
                    for rounds in (1, 2):
                        _, _, flag = dev_orth(e, Y, rounds)
                        assert flag == j + 1, (l, bad, j, rounds, flag)
            Q, _, flag = dev_orth(e, orth_input(N, l), 2)          # the flag does not stick to the handle
            assert flag == 0 and np.all(np.isfinite(Q))


@pytest.mark.gpu
def test_two_handles_in_one_process_both_run_the_wide_cholesky(gpca):
    """k_chol_inv_any's 129 KiB of LDS are opted in at gpca_create on the handle's device (it sat behind a process-wide static); a
    launch that is refused is an error now, not a stale Z."""
    N, l = 257, 100
    Y = orth_input(N, l)
    kappa = precondition(Y)
    got = []
    for _ in range(2):
        with open_carrier(gpca, N) as e:
            Q, s, flag = dev_orth(e, Y, 2)
            assert flag == 0
            fr = report(f"handle {len(got)} N={N} l={l}", orth_fractions(Y, Q, 2, kappa))
            assert inside(fr), fr
            got.append(Q)
    assert np.array_equal(got[0].view(np.uint64), got[1].view(np.uint64))


@pytest.mark.gpu
def test_refine_reports_a_non_finite_start(gpca, carriers):
    """k = 3: L = 32, so every kernel downstream of the flag has bounded loops (the Jacobi's 40 sweeps at worst; its own comment: a NaN
    input ends after the first).  The flag travels through the result block to the one host wait of the call."""
    N = 257
    e = carriers(N)
    S0 = np.random.default_rng(11).standard_normal((N, 3))
    bad = S0.copy()
    bad[100, 1] = np.inf
    with pytest.raises(gpca.GpcaError) as err:
        e.refine(bad)
    assert err.value.status == _lib.GPCA_ERR_NOT_CONVERGED and "pivot 1 of the 3-column sketch is not finite" in str(err.value), str(err.value)
    e.refine(S0)                         # the flag does not stick to the handle
    assert np.all(np.isfinite(e.scores(f64=True))) and np.all(np.isfinite(e.loadings()))


# (N, l, k, pair): every pair with either row first; zmode 1 both times (the sign reaches the loadings bit for bit), zmode 0 once
SIGN_CASES = [(12588, 32, 32, (0, 1)), (12588, 20, 12, (255, 256)), (12588, 64, 64, (12287, 12288)), (12588, 32, 20, (12287, 12288)),
              (12588, 33, 33, (5, 12587)), (12588, 64, 40, (255, 256)),
              (4400, 100, 90, (0, 1)), (4400, 128, 128, (1023, 1024)), (4400, 65, 65, (4095, 4096)), (4400, 100, 100, (5, 4399))]


@pytest.mark.gpu
@pytest.mark.parametrize("N,l,k,pair", SIGN_CASES)
def test_scores_and_the_sign_rule(carriers, N, l, k, pair):
    e = carriers(N)
    for neg_first, zmode in ((False, 1), (True, 1), (False, 0)):
        case = TailCase(N, l, k, zmode, pair=pair, neg_first=neg_first)
        fr = report(f"tail N={N} l={l} k={k} zmode={zmode} pair={pair} neg_first={neg_first}", tail_fractions(case, dev_tail(e, case), eigen=N <= 4400 and zmode == 0))
        assert inside(fr), (l, k, pair, neg_first, zmode, fr)


EIGEN_SHAPES = [(1, 1), (31, 31), (31, 9), (32, 32), (32, 1), (33, 33), (33, 20), (64, 64), (64, 63), (100, 90)]
KEEP_90 = (np.arange(M_CARRIER) % 13 >= 4).astype(np.uint8)          # 40 of the 130 rows dropped


@pytest.mark.gpu
@pytest.mark.parametrize("dropped", [False, True])
def test_eigen_step_as_the_product_calls_it(gpca, dropped):
    N = 300
    keep = KEEP_90 if dropped else None
    assert not dropped or int(KEEP_90.sum()) == 90
    worst = {}
    with open_carrier(gpca, N, keep=keep) as e:
        for l, k in EIGEN_SHAPES:
            if dropped and l > 90:
                continue
            for zmode in (0, 1):
                for zero_col in ((None, l // 2) if l > 1 else (None,)):
                    if zero_col is not None and k < l:
                        continue           # (the zero singular value is the last one: seen with k = l)
                    case = TailCase(N, l, k, zmode, keep=keep, zero_col=zero_col)
                    out = dev_tail(e, case)
                    fr = report(f"eigen N={N} l={l} k={k} zmode={zmode} zero_col={zero_col} dropped={dropped}", tail_fractions(case, out))
                    assert inside(fr), (l, k, zmode, zero_col, fr)
                    if zero_col is not None:
                        assert out["sv"][-1] == 0.0 or zmode == 1, out["sv"][-3:]
                    for name, v in fr.items():
                        worst[name] = max(worst.get(name, 0.0), v)
    print(f"eigen dropped={dropped}: worst fractions " + "  ".join(f"{n} {v:.3g}" for n, v in sorted(worst.items())))


# ---- (c) the device recipe in numpy, and its mutants --------------------------------------------------------------------------------------
def sim_gram(X, drop_last_block=False):
    rows = X.shape[0]
    rpb = gram_rows_per_block(rows)
    parts = [X[r0:r0 + rpb].T @ X[r0:r0 + rpb] for r0 in range(0, rows, rpb)]
    if drop_last_block and len(parts) > 1:
        parts = parts[:-1]
    W = np.zeros((X.shape[1],) * 2)
    for p in parts:
        W = W + p
    return W


def sim_chol_inv(W, tol=CHOL_TOL, zero_dependent=True, drop_last_col=False):
    """(Z = R^-1, flag): right-looking Cholesky of the upper triangle with the rank rule of k_chol_inv, back substitution row by row"""
    n = W.shape[0]
    R, dinv, flag = np.array(W, np.float64), np.zeros(n), 0
    with np.errstate(all="ignore"):
        for j in range(n):
            piv, d0 = R[j, j], W[j, j]
            if not (np.isfinite(piv) and np.isfinite(d0)):
                flag = flag or j + 1
                piv = 1.0
            dependent = not (piv > tol * d0)
            if dependent and not zero_dependent:
                dependent, piv = False, (abs(piv) if piv != 0 else 1.0)
            dinv[j] = 0.0 if dependent else 1.0 / np.sqrt(piv)
            R[j, j:] = R[j, j:] * dinv[j]
            R[j, j] = piv * dinv[j]
            R[j + 1:, j + 1:] -= np.outer(R[j, j + 1:], R[j, j + 1:])
        R = np.triu(R)
        X = np.zeros((n, n))
        for i in range(n - 1, -1, -1):
            acc = -(R[i, i + 1:] @ X[i + 1:])
            acc[i] += 1.0
            X[i] = acc * dinv[i]
    X = np.triu(X)
    if drop_last_col:
        X[:, -1] = 0.0
    return X, flag


def sim_orth(Y, rounds=2, mutant=None):
    Q, flag = np.array(Y, np.float64), 0
    if mutant == "one_round":
        rounds = 1
    kw = {"tol_1e-9": dict(tol=1e-9), "dependent_kept": dict(zero_dependent=False), "rinv_last_col": dict(drop_last_col=True)}.get(mutant, {})
    with np.errstate(all="ignore"):
        for _ in range(rounds):
            Z, f = sim_chol_inv(sim_gram(Q, drop_last_block=mutant == "gram_last_block"), **kw)
            flag = flag or f
            Q = Q @ Z
    return Q, Q.sum(axis=0), flag


ORTH_MUTANTS = ["one_round", "gram_last_block", "dependent_kept", "tol_1e-9", "rinv_last_col"]


def sim_sign(S, wide, mutant=None):
    """the sign per column: +1 unless the first row of maximal |score| is negative.  wide: k_col_sign (thread t walks rows t, t + 1024, ..;
    a tree folds the threads); else k_scores' 256-row chunks dealt to scores_num_parts workgroups and the fold of k_scores_sign."""
    N, K = S.shape
    A = np.abs(S)
    sign = np.ones(K)
    for c in range(K):
        a = A[:, c]
        m = a.max()
        ties = np.flatnonzero(a == m)
        if mutant == "tie_later":
            r = ties[-1]
        elif mutant == "tie_boundary":
            if wide:                     # the tree keeps the lower THREAD on a tie, not the lower row
                own = {}
                for t in ties:
                    own.setdefault(t % 1024, t)
                r = own[min(own)]
            else:                        # the fold keeps the earlier WORKGROUP on a tie, not the lower row
                parts = scores_num_parts(N)
                own = {}
                for t in ties:
                    own.setdefault((t // 256) % parts, t)
                r = own[min(own)]
        else:
            r = ties[0]
        sign[c] = -1.0 if S[r, c] < 0 else 1.0
    return sign


def sim_tail(case, mutant=None):
    l, k, zmode, L = case.l, case.k, case.zmode, padded(case.l)
    Bk = np.where(case.keep[:, None] != 0, case.B, np.float32(0)).astype(np.float64)
    Cm = sim_gram(Bk if zmode == 0 else case.Q)
    w, V = np.linalg.eigh((Cm + Cm.T) / 2)
    w, V = w[::-1].copy(), V[:, ::-1].copy()
    for c in range(l):                   # the eigenvector of an exactly zero row / column of C is e_c: LAPACK returns it, make it exact
        if not np.any(Cm[c]):
            w[np.argmax(np.abs(V[c]))] = 0.0
    order = np.argsort(-w, kind="stable")
    w, V = w[order], V[:, order]
    sv = np.sqrt(np.maximum(w, 0.0))
    eig = w[:k] if mutant == "eig_no_denom" else w[:k] / case.denom
    with np.errstate(all="ignore"):
        if zmode == 0:
            Z0 = V[:, :k] * sv[:k]
            Z1 = V[:, :k] / sv[:k] if mutant == "z1_no_guard" else np.where(sv[:k] > 0, V[:, :k] / np.where(sv[:k] > 0, sv[:k], 1), 0.0)
        else:
            Z0 = Z1 = V[:, :k]
        S = case.Q @ Z0
        sign = sim_sign(S, L > 64, mutant)
        S = S * sign
        load = (Bk[case.rows] @ (Z1 if mutant == "loadings_unsigned" else Z1 * sign)).astype(np.float32)
    return {"scores64": S, "scores32": S.astype(np.float32), "sv": sv, "eig": eig, "loadings": load}


TAIL_MUTANTS = ["tie_later", "tie_boundary", "z1_no_guard", "loadings_unsigned", "eig_no_denom"]
TEETH_ORTH = [(N, l) for N in (33, 257, 1000, 64, 128) for l in ORTH_SHAPES[N] if l in (2, 31, 32, 33, 64, 65, 100, 128)]


def test_restated_plan_reaches_the_branches_the_shapes_are_chosen_for():
    assert [gram_rows_per_block(n) for n in (33, 255, 256, 257, 1000)] == [32] * 5 and gram_num_parts(33) == 2 and gram_num_parts(257) == 9
    assert gram_num_parts(1000) == 32 and gram_num_parts(8193) < gram_num_parts(16400) <= 64 < gram_num_parts(262145)
    assert tail_num_parts(16400) <= 512 < tail_num_parts(33000)                      # kFinishQFoldMax
    assert scores_num_parts(12588) == 48 and 12288 // 256 == 48 and scores_num_parts(4400) == 18
    assert all(8 * kappa_for(N, l) * np.sqrt(g_of(N, l)) <= 1 and (l == 1 or kappa_for(N, l) >= 1e3) for N, ls in ORTH_SHAPES.items() for l in ls)
    assert kappa_for(262145, 20) == 1e3 and 8e3 * np.sqrt(g_of(262145, 20)) <= 1


def test_teeth_simulator_and_householder_sit_inside_the_orth_bars():
    worst = {}
    for N, l in TEETH_ORTH:
        Y = orth_input(N, l)
        kappa = precondition(Y)
        Qh, Rh = np.linalg.qr(Y)
        Qh = Qh * np.where(np.diag(Rh) < 0, -1.0, 1.0)
        for who, (Q, rounds) in {"householder": (Qh, 2), "simulator": (sim_orth(Y, 2)[0], 2), "simulator, one round": (sim_orth(Y, 1)[0], 1)}.items():
            fr = orth_fractions(Y, Q, rounds, kappa)
            if who.startswith("simulator"):
                fr["s"] = s_fraction(Q, Q.sum(axis=0))
            assert inside(fr), (who, N, l, fr)
            for name, v in fr.items():
                worst[(who, name)] = max(worst.get((who, name), 0.0), v)
    print("largest fractions: " + "  ".join(f"{w} {n} {v:.3g}" for (w, n), v in sorted(worst.items())))


def test_teeth_every_orth_mutant_leaves_a_bar_or_fails_an_exact_check():
    margins = {}
    for N, l in TEETH_ORTH:
        if l < 2:
            continue
        Y = orth_input(N, l)
        kappa = precondition(Y)
        for m in ("one_round", "gram_last_block", "rinv_last_col"):
            Q, _, flag = sim_orth(Y, 2, m)
            margins.setdefault(m, []).append((max(orth_fractions(Y, Q, 2, kappa).values()), N, l))
    for l in CONTRACT_L:
        N = 257
        for kind in ("duplicate", "zero"):
            Y, j, rest = dependent_inputs(N, l, kind)
            Q, _, flag = sim_orth(Y, 2)
            assert flag == 0 and np.all(Q[:, j] == 0.0) and inside(orth_fractions(Y[:, rest], Q[:, rest], 2)), (l, kind)
            if kind == "duplicate":      # (a zero column stays zero whatever the rule)
                Q, _, flag = sim_orth(Y, 2, "dependent_kept")
                margins.setdefault("dependent_kept", []).append((np.inf if not np.all(Q[:, j] == 0.0) else 0.0, N, l))
        Y, j = small_pivot_input(N, l)
        Q, _, flag = sim_orth(Y, 2)
        assert flag == 0 and np.linalg.norm(Q[:, j]) > 0.5
        Q, _, flag = sim_orth(Y, 2, "tol_1e-9")
        margins.setdefault("tol_1e-9", []).append((np.inf if not np.linalg.norm(Q[:, j]) > 0.5 else 0.0, N, l))
        for bad in (np.inf, np.nan):
            Y = orth_input(N, l)
            Y[N // 2, l // 2] = bad
            assert sim_orth(Y, 2)[2] == l // 2 + 1
    for l in (32, 64, 128):
        Y, j, rest = dependent_inputs(l, l, "centred")
        Q, _, flag = sim_orth(Y, 2)
        assert flag == 0 and np.all(Q[:, j] == 0.0) and inside(orth_fractions(Y[:, rest], Q[:, rest], 2)), l
        Q, _, _ = sim_orth(Y, 2, "dependent_kept")
        margins["dependent_kept"].append((np.inf if not np.all(Q[:, j] == 0.0) else 0.0, l, l))
    assert sorted(margins) == sorted(ORTH_MUTANTS)
    for m, rows in margins.items():
        weakest = min(rows)
        print(f"mutant {m}: weakest at N = {weakest[1]}, l = {weakest[2]}: {weakest[0]:.3g} x its bar")
        assert weakest[0] > 1.0, (m, weakest)


TEETH_TAIL = [(12588, 20, 12, (12287, 12288)), (12588, 20, 20, (255, 256)), (4400, 65, 65, (4095, 4096)), (4400, 100, 90, (1023, 1024))]


def test_teeth_simulated_tail_sits_inside_the_bars_and_every_mutant_leaves_them():
    caught = {m: 0 for m in TAIL_MUTANTS}
    worst = {}
    for N, l, k, pair in TEETH_TAIL:
        for neg_first, zmode in ((False, 1), (True, 1), (False, 0)):
            case = TailCase(N, l, k, zmode, pair=pair, neg_first=neg_first)
            fr = tail_fractions(case, sim_tail(case), eigen=N <= 4400 and zmode == 0)
            assert inside(fr), (N, l, k, zmode, fr)
            for name, v in fr.items():
                worst[name] = max(worst.get(name, 0.0), v)
            for m in ("tie_later", "tie_boundary", "loadings_unsigned", "eig_no_denom"):
                bad = tail_fractions(case, sim_tail(case, m), eigen=False)
                if m == "tie_boundary" and pair == (255, 256):
                    # blind where the fold order happens to agree with the row order (workgroups 0 and 1): what the wrapped chunk
                    # (12 287, 12 288) and the strides of k_col_sign are in the case list for
                    assert inside(bad), (m, N, l, pair, neg_first, zmode, bad)
                    continue
                assert not inside(bad), (m, N, l, pair, neg_first, zmode, bad)
                caught[m] += 1
    for l, k in [(31, 31), (33, 33), (100, 100)]:
        for zmode in (0, 1):
            case = TailCase(300, l, k, zmode, zero_col=l // 2)
            fr = tail_fractions(case, sim_tail(case))
            assert inside(fr), (l, zmode, fr)
            for name, v in fr.items():
                worst[name] = max(worst.get(name, 0.0), v)
            if zmode == 0:
                assert not inside(tail_fractions(case, sim_tail(case, "z1_no_guard"))), l
                caught["z1_no_guard"] += 1
    print("largest fractions of the unmutated simulator: " + "  ".join(f"{n} {v:.3g}" for n, v in sorted(worst.items())))
    print("cases that caught each mutant: " + "  ".join(f"{m} {n}" for m, n in caught.items()))
    assert all(n > 0 for n in caught.values()), caught
