"""K1, T = r o (G Q) + b s^T, of every kernel that computes it, held per element to a bar derived from its arithmetic -- through the loadings.

THE IDENTITY.  Step 3 of gpca_rsvd is B = A Q by ONE K1 sweep (stage_AQ(h, 0)), then the l x l eigenproblem of B^T B -> V, sv, then
    scores = Q V_k diag(sv) (f64),   loadings = B V_k diag(sign / sv) (f32, launch_rightmul_gather_f32: f64 accumulation, one f32 store)
with the same V_k, sv and sign.  So, whatever V_k is (it need not even be orthogonal), for every PCA SNP row i and column c < k
    loadings[i][c] = ( sum_n A[i][n] scores[n][c] ) / sv[c]^2,      A[i][n] = (g - mu_i) / sigma_i      (``k1_truth``: plain f64 on the uploaded bytes)
and the only device work between the two sides is that K1 sweep and the small right-multiplication.  A fault COMMON to scores and
loadings (a wrong Q, a wrong V) is out of this test's reach by construction: the oracle parity tests of test_gpu_parity.py cover that.
mu, sigma are the CPU's (oracle.snp_stats); the device's must equal them (mu bit for bit, sigma within 1 ulp -- a row whose sigma is
1 ulp off gets 2 u32 |loading| more bar, nothing is read back and trusted).

gpca_refine does NOT satisfy that identity for k > 1: its scores are A^T L W of a SECOND pass (gpca_rsvd.cpp, gpca_refine: stage_AtT_local
after the CholeskyQR2 of B), so A scores = A A^T loadings.  What its K1 sweep leaves observable: Q = orth(S0) is known on the CPU (CholeskyQR2's
Q = Householder QR's with a positive diagonal of R), L = orth(B) by CholeskyQR2 in f32 over the rows, loadings = L W.  So
    k = 1:  loadings = A q / |A q| up to sign, element by element (``refine1_bar``);
    k > 1:  the columns of the loadings lie in span(A Q): the residual (I - P) loadings, P the f64 projector on span(A Q), is (I - P) dB R^-1 W
            and is bounded row by row (``refine_span_bar``).  s0 has a non-zero mean, so the b s^T term of K1 is as large as r (G Q).

THE BAR (``k1_bar``), u32 = 2^-24, u64 = 2^-53, S = digit_scale(nd), l = k + oversample, L = the padded sketch (32 / 64 / 128), per row i:
  quantisation of Q (exact path; fold_quantize_i8.hip: q = rint(Q * (S / colmax_j)) in f64, two roundings of a value below S in front of the
    rint): every entry of Q is off by at most (0.5 + 2 u64 S) colmax_j / S, the integer sum is exact, so the row dB_i has
    |dB_i|_2 <= r_i (sum_n g_in) (0.5 + 2 u64 S) / S * sqrt(l) * cm,   cm >= every colmax_j.
  f32 roundings of B_ij = fma(r_i, f32(int * qscale), fmul(b_i, s32_j)) against the truth: three act on r_i (G Q)_ij (r = f32(1 / sigma), the
    f32 of int * qscale, the fma) and five on b_i s_j (b = f32(-mu r) carries two, s32, the fmul, the fma):
    |dB_i|_2 <= u32 (3 RG_i + 5 BS_i) (1 + 8 u32),   RG_i >= |r_i (G Q)_i.|_2,  BS_i >= |b_i| |s|_2.
  GPCA_PREC_F32_MFMA (gemm_f32.hip: Q rounded to f32, ONE accumulator per element, a chain of Npad = 256 ceil(N / 256) fmas in sample order,
    then ri * (acc * 2^9) + bi * sj): no quantisation term;  |dB_i|_2 <= u32 ((Npad + 1) AG_i + 4 RG_i + 5 BS_i) (1 + 8 u32),
    AG_i >= r_i |(sum_n g_in |Q_nj|)_j|_2.
  Q, V are not outputs; what hides is bounded by what shows.  |sum_j dB_ij V_jc| <= |dB_i|_2 (a column of V has norm 1).  oversample = 0: V is
    square, Q = P V^T with P = scores diag(1 / sv), so |Q_nj| <= |P_n.|_2 (cm = rho = max_n |P_n.|_2), s = V (P^T 1) (|s|_2 = |P^T 1|_2), B = (truth diag(sv)) V^T
    (|B_i.|_2 = |truth_i. o sv|_2, RG_i <= that + BS_i), AG_i <= r_i sqrt(l) min(rho sum_n g_in, |g_i|_2).  oversample > 0: only cm <= 1,
    |s|_2 <= sqrt(N_eff), RG_i <= r_i |g_i|_2 (Q has orthonormal columns), AG_i <= r_i sqrt(l) |g_i|_2 hold: the bar is looser there, honestly so.
  the f32 store of the loading: u32 |truth_ic|.      scores, sv (f64 device results, dot products of L terms) and the truth's own f64 sum:
    u64 ((L + 2) (sum_n |A_in|) cm / sv_c + (N + 2 (L + 2)) sum_n |A_in scores_nc| / sv_c^2).
  bar_ic = (the |dB_i|_2 terms) / sv_c + those.  Every factor is a count read from the code, a unit roundoff or a formula over the inputs.
With a sample mask the sums run over the masked samples (the other rows of Q and of the scores are exactly zero: asserted).

TEETH (CPU, unmarked): ``simulate_k1`` quantises a given orthonormal Q as fold_quantize_i8.hip does, takes the integer dot, the f32 epilogue,
then V, sv from its own B^T B, and goes through the same check as the device.  Seven mutants (``MUTANTS``) must each put an element over the
bar on the device tests' own generator, nd = 3 and 4, M in {33, 4097}; the unmutated simulator and the oracle's own f64 randomized PCA must sit
inside it.  The teeth inputs keep every row (l = 30 or 33 of 33 rows) and have 1025 samples at both row counts, so that on packed rows the
last 1024-sample unit holds one sample and not all of them; the device inputs drop some rows.  GPCA_PREC_F32_MFMA has teeth of its own
(``simulate_k1_f32``: Q in f32, one f32 chain per element): last row unit, last sample block, r / b of the next row through gpca_rsvd's
identity, b s^T left out through both refine checks, the second column tile taking the first tile's s32 through the k = 33 one.

Not reached, and why: for k > 1 the refine bar sees only what K1 puts OUTSIDE span(A Q) (with 33 rows and k = 33 that is nothing, so the
k = 33 teeth run at 4097 rows only); with oversample > 0 Q is hidden, the bar rests on worst-case bounds and a defect of the lowest digit plane
stays under it; on GPCA_PREC_F32_MFMA the chain term u32 Npad AG_i is a worst case that grows with N: at N = 10 000, oversample 10 that
mode's bar is 0.6 |loading| (median), so there only gross defects show.  Streamed panels exist on the exact path only (rsvd_preflight).

Measured on one MI355X, the largest fraction of the bar over every case, row and column (each test prints its own with -s):
    gpca_rsvd     int8 0.76, 2-bit (3 planes) 0.89, 2-bit (4 planes) 0.76 -- all three at k = l = 1, where four f32 roundings can align and the bar
                  is four unit roundoffs; f32 MFMA 0.027 on int8 and on 2-bit rows (the chain term is a worst case)
                  full size (1M x 10k, k = 20 + 10; check (7) of test_gpu_parity._full_size_case): 0.037 / 0.0027 / 0.037, f32 MFMA 0.0002
    gpca_refine   k = 1: int8 0.30, 2-bit (3 planes) 0.33, 2-bit (4 planes) 0.30, f32 MFMA 0.014 on int8 and on 2-bit rows
                  k = 33, span residual: 0.027 / 0.0099 / 0.027, f32 MFMA 0.00027
One value-only defect compiled into k_gq_i8 on a scratch copy (the lowest digit plane of Q times 0; GPCA_CFG_SIMPLE_KERNELS, int8 rows), run once:
every oversample = 0 case went red (2.4 x the bar at k = l = 64), the oversample = 10 cases stayed at 0.6 - 0.75 of their looser bar, and
test_rsvd_parity_i8 on the same kernels stayed green at its 1e-4."""
import threading

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from test_gpu_exact_pass import digit_scale, int_dot, quantize, split_digits

U64, U32 = 2.0 ** -53, 2.0 ** -24
MISSING = -127
QC = (0.98, 0.0, 1.0)                 # call rate 0.98 (drops the rows with planted missing calls), no MAF or HWE filter
# mode -> (precision, storage, digit_planes argument, planes in use (0: f32), packed rows)
MODES = {"int8": (_lib.PREC_I8_EXACT, _lib.STORE_INT8, 0, 4, False), "2bit": (_lib.PREC_I8_EXACT, _lib.STORE_2BIT, 0, 3, True),
         "2bit4": (_lib.PREC_I8_EXACT, _lib.STORE_2BIT, 4, 4, True), "f32": (_lib.PREC_F32_MFMA, _lib.STORE_INT8, 0, 0, False),
         "f32_2bit": (_lib.PREC_F32_MFMA, _lib.STORE_2BIT, 0, 0, True)}
EXACT = ["int8", "2bit", "2bit4"]


def padded_sketch(l):
    return 32 if l <= 32 else (64 if l <= 64 else 128)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def make_genotypes(M, N, seed, drop=True):
    """Seeded dosages: allele frequencies log-uniform from a singleton's 1 / (2 N) to 0.5, three planted populations (a fifth of the rows
    differ strongly between them: the leading singular values stand clear of the bulk), row 0 one het call (the largest r a kept row can
    have), row M - 1 at frequency 0.5.  drop: every 7th row (3, 10, ..) gets missing calls in more than 2 % of its samples and leaves at QC;
    monomorphic rows leave by themselves.  No kept row has a missing call."""
    rng = np.random.default_rng(seed)
    pop = rng.integers(0, 3, N)
    p = np.exp(rng.uniform(np.log(0.5 / N), np.log(0.5), size=M))
    shift = np.where(rng.random((M, 1)) < 0.2, np.exp(rng.normal(0.0, 0.7, size=(M, 3))), 1.0)
    pp = np.clip(p[:, None] * shift, 0.0, 0.5)[:, pop]
    G = (rng.random((M, N)) < pp).astype(np.int8) + (rng.random((M, N)) < pp).astype(np.int8)
    G[0] = 0; G[0, N // 3] = 1
    G[M - 1] = (rng.random(N) < 0.5).astype(np.int8) + (rng.random(N) < 0.5).astype(np.int8)
    if drop:
        nmiss = int(np.ceil(0.02 * N)) + 1
        for i in range(3, M - 1, 7):
            G[i, rng.choice(N, nmiss, replace=False)] = MISSING
    else:                                                  # every row stays: a row that came out monomorphic gets one het call
        for i in np.flatnonzero(G.max(axis=1) == G.min(axis=1)):
            G[i, rng.integers(0, N)] = 1
    return G


def cpu_stats(oracle, G):
    st = oracle.snp_stats(G, G.shape[1], *QC)
    rows = np.flatnonzero(st["keep"])
    assert not np.any(G[rows] == MISSING)
    return st["mu"], st["sigma"], rows


def _chunks(n, N):
    step = max(1, (1 << 24) // max(N, 1))
    return [(a, min(n, a + step)) for a in range(0, n, step)]


# ---- the truth and the bar ---------------------------------------------------------------------------------------------------------------
def k1_truth(G, mu, sigma, rows, scores, sv, mask=None):
    """[n_pca][k] f64: ( sum_n A[i][n] scores[n][c] ) / sv[c]^2 over the PCA SNP rows, chunked over rows (no M x N f64 array)"""
    scores = np.asarray(scores, np.float64)
    k = scores.shape[1]
    if mask is not None:
        scores = scores * np.asarray(mask, bool)[:, None]
    out = np.empty((len(rows), k))
    for a, b in _chunks(len(rows), G.shape[1]):
        rr = rows[a:b]
        A = (G[rr].astype(np.float64) - mu[rr].astype(np.float64)[:, None]) / sigma[rr].astype(np.float64)[:, None]
        out[a:b] = A @ scores
    return out / np.asarray(sv, np.float64)[:k] ** 2


def row_sums(G, mu, sigma, rows, scores, sv, mask=None):
    """per PCA SNP row: sum_n g, |g|_2, sum_n |A_in| (over the masked samples) and [n_pca][k] sum_n |A_in scores_nc| / sv_c^2"""
    k = scores.shape[1]
    m = np.ones(G.shape[1], bool) if mask is None else np.asarray(mask, bool)
    g1, g2, a1 = np.empty(len(rows)), np.empty(len(rows)), np.empty(len(rows))
    absacc = np.empty((len(rows), k))
    asc = np.abs(scores) * m[:, None]
    for a, b in _chunks(len(rows), G.shape[1]):
        rr = rows[a:b]
        g = G[rr].astype(np.float64) * m[None, :]
        A = np.abs((G[rr].astype(np.float64) - mu[rr].astype(np.float64)[:, None]) / sigma[rr].astype(np.float64)[:, None]) * m[None, :]
        g1[a:b], g2[a:b], a1[a:b] = g.sum(axis=1), np.sqrt((g * g).sum(axis=1)), A.sum(axis=1)
        absacc[a:b] = A @ asc
    return g1, g2, a1, absacc / np.asarray(sv, np.float64)[:k] ** 2


def k1_bar(G, mu, sigma, rows, scores, sv, l, nd, truth, mask=None, sigma_ulps=None):
    """[n_pca][k]: the module docstring's bar.  nd = 3 / 4: the exact path; nd = 0: GPCA_PREC_F32_MFMA."""
    scores, sv = np.asarray(scores, np.float64), np.asarray(sv, np.float64)
    N, k = scores.shape
    svk = sv[:k]
    L = padded_sketch(l)
    n_eff = N if mask is None else int(np.sum(np.asarray(mask, bool)))
    g1, g2, a1, absacc = row_sums(G, mu, sigma, rows, scores, svk, mask)
    r = 1.0 / sigma[rows].astype(np.float64)
    b = np.abs(mu[rows].astype(np.float64)) * r
    if l == k:                                             # oversample = 0: what hides is a rotation of what shows
        P = scores / svk
        cm = float(np.max(np.sqrt(np.sum(P * P, axis=1))))
        s2 = float(np.linalg.norm(P.sum(axis=0)))
        BS = b * s2
        RG = np.sqrt(np.sum((truth * svk) ** 2, axis=1)) + BS
        AG = r * np.sqrt(l) * np.minimum(cm * g1, g2)
    else:
        cm, BS, RG, AG = 1.0, b * np.sqrt(n_eff), r * g2, r * np.sqrt(l) * g2
    if nd:
        S = digit_scale(nd)
        dB = r * g1 * ((0.5 + 2 * U64 * S) / S) * np.sqrt(l) * cm + U32 * (3 * RG + 5 * BS) * (1 + 8 * U32)
    else:
        npad = (N + 255) // 256 * 256
        dB = U32 * ((npad + 1) * AG + 4 * RG + 5 * BS) * (1 + 8 * U32)
    bar = dB[:, None] / svk[None, :] + U32 * np.abs(truth)
    bar += U64 * ((L + 2) * a1[:, None] * cm / svk[None, :] + (N + 2 * (L + 2)) * absacc)
    if sigma_ulps is not None:
        bar += 2 * U32 * sigma_ulps[:, None] * np.abs(truth)
    return bar


def check(load, truth, bar, what):
    """every element against the bar; returns the worst fraction of it"""
    load = np.asarray(load, np.float64)
    assert load.shape == truth.shape == bar.shape and np.all(np.isfinite(load)), what
    d = np.abs(load - truth)
    frac = float(np.max(np.where(bar > 0, d / np.where(bar > 0, bar, 1), np.where(d > 0, np.inf, 0)), initial=0))
    typical = float(np.median(bar / np.maximum(np.abs(truth), 1e-300)))
    print(f"{what}: max |loading - truth| / bar = {frac:.3g}   (median bar / |loading| = {typical:.2g})")
    assert np.all(d <= bar), f"{what}: {frac:.3g} of the bar, worst element {np.unravel_index(np.argmax(d / np.maximum(bar, 1e-300)), d.shape)}"
    return frac


def orth_as_cholqr(S0):
    """orth(S0) as CholeskyQR makes it: Q = S0 R^-1 with R upper triangular, positive diagonal"""
    Q, R = np.linalg.qr(np.asarray(S0, np.float64))
    return Q * np.where(np.diag(R) < 0, -1.0, 1.0)[None, :]


def known_q_dB(G, mu, sigma, rows, S0, nd):
    """per element |dB_ij| of one K1 sweep with a KNOWN Q = orth(S0) (the refine cases), and B = A Q in f64.  nd = 3 / 4: quantisation + the
    f32 roundings of the exact path; nd = 0 (GPCA_PREC_F32_MFMA): u32 ((Npad + 1) r sum_n g |Q_nj| + 4 |r (G Q)_ij| + 5 |b_i s_j|).  The
    device's Q is CholeskyQR2's in f64: orthonormal to u64 N k (Gram and triangular solve are sums of N and k terms), off the exact factor by at
    most u64 N k cond(S0)^2 per entry of a unit column, which A carries into B as u64 N k cond(S0)^2 sum_n |A_in|."""
    Q = orth_as_cholqr(S0)
    N, k = Q.shape
    Gk = G[rows].astype(np.float64)
    r = 1.0 / sigma[rows].astype(np.float64)
    b = -mu[rows].astype(np.float64) * r
    GQ, s = Gk @ Q, Q.sum(axis=0)
    rg, bs = np.abs(r[:, None] * GQ), np.abs(b[:, None] * s[None, :])
    if nd:
        S = digit_scale(nd)
        colmax = np.max(np.abs(Q), axis=0)
        dB = (r * Gk.sum(axis=1))[:, None] * ((0.5 + 2 * U64 * S) / S) * colmax[None, :] + U32 * (3 * rg + 5 * bs) * (1 + 8 * U32)
    else:
        npad = (N + 255) // 256 * 256
        dB = U32 * ((npad + 1) * r[:, None] * (Gk @ np.abs(Q)) + 4 * rg + 5 * bs) * (1 + 8 * U32)
    a1 = np.sum(np.abs(Gk * r[:, None] + b[:, None]), axis=1)
    dB = dB + (U64 * N * k * np.linalg.cond(np.asarray(S0, np.float64)) ** 2 * a1)[:, None]
    return dB, r[:, None] * GQ + b[:, None] * s[None, :]


def refine1_bar(G, mu, sigma, rows, s0, nd):
    """k = 1: (truth = A q / |A q|, bar).  |d loading_i| <= dB_i / |B| + |truth_i| |dB|_2 / |B| (the norm) + 3 u32 |truth_i| (two in-place f32
    scalings of CholeskyQR2 and the f32 store of L W)"""
    dB, B = known_q_dB(G, mu, sigma, rows, s0.reshape(-1, 1), nd)
    nrm = float(np.linalg.norm(B))
    truth = B / nrm
    return truth, dB / nrm + np.abs(truth) * (float(np.linalg.norm(dB)) / nrm + 3 * U32)


def refine_span_bar(G, mu, sigma, rows, S0, nd):
    """k > 1: (Qb = an orthonormal basis of span(A Q), per-row bar on |((I - P) loadings)_ic|).  loadings = (B + dB) R^-1 W through two f32
    in-place scalings and an f32 store (each rounds an element of a matrix whose rows have the norm |Qb_i.|_2, 3 u32 in all), so
    |((I - P) loadings)_i.| <= (|dB_i.|_2 + |Qb_i.|_2 |dB|_F) / sigma_min(B) + 3 u32 (|Qb_i.|_2 + |Qb_i.|_2 sqrt(k))"""
    dB, B = known_q_dB(G, mu, sigma, rows, S0, nd)
    Qb, _ = np.linalg.qr(B)
    smin = float(np.linalg.svd(B, compute_uv=False)[-1])
    qn, dn = np.sqrt(np.sum(Qb * Qb, axis=1)), np.sqrt(np.sum(dB * dB, axis=1))
    k = S0.shape[1]
    return Qb, (dn + qn * float(np.linalg.norm(dB))) / smin + 3 * U32 * qn * (1 + np.sqrt(k))


# ---- the simulator and its mutants (CPU) ---------------------------------------------------------------------------------------------------
MUTANTS = ["last_unit_out", "last_sample_block_out", "drop_lowest_plane", "base_off_by_one", "bs_left_out", "rb_of_next_row", "second_half_first_qscale"]


def simulate_k1(G, mu, sigma, rows, Q, nd, packed=False, mutate=None):
    """B [n_pca][l] f32 as the exact-path K1 kernels make it from an orthonormal Q (f64): digit planes of rint(Q * S / colmax), the integer
    dot, gq = f32(int * qscale), B = fma(r, gq, fmul(b, s32))"""
    Gk = G[rows].astype(np.int64)
    n, N = Gk.shape
    l = Q.shape[1]
    sg = sigma[rows].astype(np.float32)
    r = (np.float32(1) / sg).astype(np.float32)
    b = (-mu[rows].astype(np.float32) * r).astype(np.float32)
    if mutate == "rb_of_next_row":
        r, b = np.roll(r, -1), np.roll(b, -1)
    q, scale, _ = quantize(Q, nd)
    if mutate == "second_half_first_qscale":
        scale = scale.copy(); scale[32:] = scale[:l - 32]
    if mutate == "last_sample_block_out":
        unit = 1024 if packed else 256
        Gk = Gk.copy(); Gk[:, unit * ((N - 1) // unit):] = 0
    dg, base = split_digits(q, nd)
    if mutate is None:
        assert np.array_equal(sum(d * base ** i for i, d in enumerate(dg)), q)
    if mutate == "drop_lowest_plane":
        dg[0] = np.zeros_like(dg[0])
    wbase = base - 1 if mutate == "base_off_by_one" else base
    isum = sum(int_dot(Gk.T, d) * wbase ** i for i, d in enumerate(dg))
    gq = (isum.astype(np.float64) * scale[None, :]).astype(np.float32)
    s32 = np.zeros(l, np.float32) if mutate == "bs_left_out" else Q.sum(axis=0).astype(np.float32)
    bs = (b[:, None] * s32[None, :]).astype(np.float32)
    B = (r.astype(np.float64)[:, None] * gq.astype(np.float64) + bs.astype(np.float64)).astype(np.float32)
    if mutate == "last_unit_out":
        B[(n - 1) // 32 * 32:] = 0
    return B


def simulate_k1_f32(G, mu, sigma, rows, Q, mutate=None):
    """B [n_pca][l] f32 as k_gq_f32 makes it: Q rounded to f32, one f32 accumulator per element walking the samples in order (g q is exact
    in f32 for g in {0, 1, 2}, so every fma rounds once), then ri * acc + bi * sj.  second_tile_first_s: the columns of the second 32-column
    tile take s32 of the first."""
    Gk = G[rows].astype(np.float32)
    n, N = Gk.shape
    l = Q.shape[1]
    r = (np.float32(1) / sigma[rows].astype(np.float32)).astype(np.float32)
    b = (-mu[rows].astype(np.float32) * r).astype(np.float32)
    if mutate == "rb_of_next_row":
        r, b = np.roll(r, -1), np.roll(b, -1)
    Q32 = Q.astype(np.float32)
    n_end = 256 * ((N - 1) // 256) if mutate == "last_sample_block_out" else N
    acc = np.zeros((n, l), np.float32)
    for s_ in range(n_end):
        acc += Gk[:, s_, None] * Q32[None, s_, :]
    s32 = Q.sum(axis=0).astype(np.float32)
    if mutate == "bs_left_out":
        s32 = np.zeros(l, np.float32)
    if mutate == "second_tile_first_s":
        s32 = s32.copy(); s32[32:] = s32[:l - 32]
    B = (r[:, None] * acc).astype(np.float32) + (b[:, None] * s32[None, :]).astype(np.float32)
    if mutate == "last_unit_out":
        B[(n - 1) // 32 * 32:] = 0
    return B.astype(np.float32)


def finish_as_rsvd(B, Q):
    """scores, loadings (f32), sv from B and Q as step 4 of gpca_rsvd makes them (k = l)"""
    B64 = B.astype(np.float64)
    w, V = np.linalg.eigh(B64.T @ B64)
    w, V = w[::-1], V[:, ::-1]
    sv = np.sqrt(np.maximum(w, 0))
    scores = (Q @ V) * sv
    sgn = np.sign(scores[np.abs(scores).argmax(axis=0), np.arange(len(sv))]); sgn[sgn == 0] = 1
    return scores * sgn, ((B64 @ V) / sv * sgn).astype(np.float32), sv


def teeth_basis(G, mu, sigma, rows, l, seed):
    """an orthonormal Q as a q = 1 randomized PCA leaves it (f64)"""
    A = (G[rows].astype(np.float64) - mu[rows].astype(np.float64)[:, None]) / sigma[rows].astype(np.float64)[:, None]
    Q, _ = np.linalg.qr(A.T @ np.random.default_rng(seed).standard_normal((len(rows), l)))
    Q, _ = np.linalg.qr(A.T @ (A @ Q))
    return Q


def refine_start(N, k, seed):
    """S0 with non-zero column means (the b s^T term of K1 is then as large as r (G Q))"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, k)) + rng.uniform(0.5, 1.5, size=k) * np.where(np.arange(k) % 2, -1.0, 1.0)


TEETH_SHAPES = {33: 1025, 4097: 1025}      # (N > 1024: on packed rows the last 1024-sample unit holds one sample, not all of them)


@pytest.mark.parametrize("M", [33, 4097])
@pytest.mark.parametrize("nd", [3, 4])
def test_the_bar_rejects_every_mutant(oracle, nd, M):
    N = TEETH_SHAPES[M]
    packed = nd == 3
    G = make_genotypes(M, N, seed=M + nd, drop=False)
    mu, sigma, rows = cpu_stats(oracle, G)
    assert len(rows) >= 33
    fr = {}
    for l, muts in ((30, MUTANTS[:4] + MUTANTS[5:6]), (33 if M == 33 else 40, MUTANTS[6:])):
        Q = teeth_basis(G, mu, sigma, rows, l, seed=nd)
        sc, ld, sv = finish_as_rsvd(simulate_k1(G, mu, sigma, rows, Q, nd, packed), Q)
        truth = k1_truth(G, mu, sigma, rows, sc, sv)
        fr[f"none(l={l})"] = check(ld, truth, k1_bar(G, mu, sigma, rows, sc, sv, l, nd, truth), f"nd={nd} M={M} l={l}: the unmutated simulator")
        for mut in muts:
            sc, ld, sv = finish_as_rsvd(simulate_k1(G, mu, sigma, rows, Q, nd, packed, mutate=mut), Q)
            truth = k1_truth(G, mu, sigma, rows, sc, sv)
            bar = k1_bar(G, mu, sigma, rows, sc, sv, l, nd, truth)
            fr[mut] = float(np.max(np.abs(ld - truth) / bar))
            print(f"nd={nd} M={M} l={l}: mutant {mut}: max |d| / bar = {fr[mut]:.3g}")
    # the refine case, k = 1: s0 with a non-zero mean
    s0 = refine_start(N, 1, seed=M)[:, 0]
    q = orth_as_cholqr(s0.reshape(-1, 1))
    truth, bar = refine1_bar(G, mu, sigma, rows, s0, nd)
    for mut in (None, "bs_left_out"):
        B = simulate_k1(G, mu, sigma, rows, q, nd, packed, mutate=mut).astype(np.float64)
        ld = (B / np.linalg.norm(B)).astype(np.float32).astype(np.float64)
        f = float(np.max(np.abs(ld * np.sign(np.sum(ld * truth)) - truth) / bar))
        print(f"nd={nd} M={M} refine k=1: mutant {mut}: max |d| / bar = {f:.3g}")
        fr["refine:" + str(mut)] = f
    assert fr["refine:None"] <= 1
    for mut in MUTANTS:
        key = "refine:bs_left_out" if mut == "bs_left_out" else mut
        assert np.isfinite(fr[key]) and fr[key] > 1, f"the bar lets the mutant '{mut}' through ({fr[key]:.3g} of it)"


@pytest.mark.parametrize("nd", [3, 4])
def test_the_oracle_alone_satisfies_the_identity(oracle, nd):
    """the reference's own f64 randomized PCA inside the bar, oversample 0 and 10 -- and inside the f32 path's bar"""
    G = make_genotypes(4097, 1025, seed=11)
    mu, sigma, rows = cpu_stats(oracle, G)
    r, b = oracle.scale_shift(mu, sigma, np.isin(np.arange(len(mu)), rows))
    for k, os_ in ((30, 0), (22, 10)):
        R = oracle.rsvd(G, G.shape[1], r, b, k, os_, 1, seed=3)
        truth = k1_truth(G, mu, sigma, rows, R["scores"], R["singular_values"])
        for planes in (nd, 0):
            bar = k1_bar(G, mu, sigma, rows, R["scores"], R["singular_values"], k + os_, planes, truth)
            # (the oracle's loadings are f64 and its r, b are the f32 ones: a subset of the roundings the bar counts)
            check(R["loadings"][rows], truth, bar, f"oracle.rsvd k={k} oversample={os_} planes={planes}")


def test_refine_bars_hold_for_the_simulator(oracle):
    """the k > 1 refine check on the CPU: orth of the simulator's B lies in span(A Q) within the bar, and leaves it when b s^T is left out"""
    G = make_genotypes(4097, 257, seed=5)
    mu, sigma, rows = cpu_stats(oracle, G)
    S0 = refine_start(257, 33, seed=2)
    Q = orth_as_cholqr(S0)
    for nd in (3, 4):
        Qb, bar = refine_span_bar(G, mu, sigma, rows, S0, nd)
        worst = {}
        for mut in (None, "bs_left_out", "second_half_first_qscale"):
            B = simulate_k1(G, mu, sigma, rows, Q, nd, mutate=mut).astype(np.float64)
            ld = np.linalg.qr(B)[0].astype(np.float32).astype(np.float64)
            res = np.abs(ld - Qb @ (Qb.T @ ld))
            worst[mut] = float(np.max(res / bar[:, None]))
            print(f"nd={nd} refine k=33 span residual: mutant {mut}: max / bar = {worst[mut]:.3g}")
        assert worst[None] <= 1 and worst["bs_left_out"] > 1 and worst["second_half_first_qscale"] > 1


@pytest.mark.parametrize("M", [33, 4097])
def test_the_f32_bar_rejects_its_mutants(oracle, M):
    """GPCA_PREC_F32_MFMA: the simulator of k_gq_f32 inside the bar, gross defects outside it -- through gpca_rsvd's identity (l = 30; there
    s = Q^T 1 is about 0, so only a refine start shows b s^T) and through both refine checks (k = 33: the second column tile's s32)"""
    N = 1025
    G = make_genotypes(M, N, seed=M, drop=False)
    mu, sigma, rows = cpu_stats(oracle, G)
    fr = {}
    Q = teeth_basis(G, mu, sigma, rows, 30, seed=1)
    for mut in (None, "last_unit_out", "last_sample_block_out", "rb_of_next_row"):
        sc, ld, sv = finish_as_rsvd(simulate_k1_f32(G, mu, sigma, rows, Q, mutate=mut), Q)
        truth = k1_truth(G, mu, sigma, rows, sc, sv)
        fr[f"rsvd:{mut}"] = float(np.max(np.abs(ld - truth) / k1_bar(G, mu, sigma, rows, sc, sv, 30, 0, truth)))
        print(f"f32 M={M} rsvd l=30: mutant {mut}: max |d| / bar = {fr[f'rsvd:{mut}']:.3g}")
    s0 = refine_start(N, 1, seed=M)[:, 0]
    truth, bar = refine1_bar(G, mu, sigma, rows, s0, 0)
    for mut in (None, "bs_left_out"):
        B = simulate_k1_f32(G, mu, sigma, rows, orth_as_cholqr(s0.reshape(-1, 1)), mutate=mut).astype(np.float64)
        ld = (B / np.linalg.norm(B)).astype(np.float32).astype(np.float64)
        fr[f"refine1:{mut}"] = float(np.max(np.abs(ld * np.sign(np.sum(ld * truth)) - truth) / bar))
        print(f"f32 M={M} refine k=1: mutant {mut}: max |d| / bar = {fr[f'refine1:{mut}']:.3g}")
    S0 = refine_start(N, 33, seed=M + 1)
    Qb, rbar = refine_span_bar(G, mu, sigma, rows, S0, 0)
    for mut in (None, "bs_left_out", "second_tile_first_s") if M > 33 else ():      # (33 columns span all of 33 rows: nothing lies outside)
        B = simulate_k1_f32(G, mu, sigma, rows, orth_as_cholqr(S0), mutate=mut).astype(np.float64)
        ld = np.linalg.qr(B)[0].astype(np.float32).astype(np.float64)
        fr[f"span:{mut}"] = float(np.max(np.abs(ld - Qb @ (Qb.T @ ld)) / rbar[:, None]))
        print(f"f32 M={M} refine k=33 span residual: mutant {mut}: max / bar = {fr[f'span:{mut}']:.3g}")
    for key, f in fr.items():
        assert np.isfinite(f) and (f <= 1 if key.endswith("None") else f > 1), f"{key}: {f:.3g} of the bar"


# ---- the device ----------------------------------------------------------------------------------------------------------------------------
_CASES = {}


def case_inputs(oracle, M, N, seed):
    """(G, mu, sigma, rows) built once per shape and shared between modes and kernel variants"""
    key = (M, N, seed)
    if key not in _CASES:
        G = make_genotypes(M, N, seed)
        mu, sigma, rows = cpu_stats(oracle, G)
        assert len(rows) < M, "QC must drop some rows (d_pca_rows gathers)"
        _CASES[key] = (G, mu, sigma, rows)
    return _CASES[key]


def device_stats(e, mu, sigma, rows):
    """run the device's QC and hold it to the CPU's: keep equal, mu bit-equal, sigma within 1 ulp; returns the rows' ulp distance (0 / 1)"""
    st = e.snp_stats(gpca.QcConfig(*QC))
    assert np.array_equal(e.pca_snp_rows(), rows)
    assert np.array_equal(st["mu"][rows], mu[rows])
    ulps = np.abs(st["sigma"][rows].astype(np.float64) - sigma[rows].astype(np.float64)) / np.spacing(sigma[rows]).astype(np.float64)
    assert np.all(ulps <= 1)
    return ulps


def open_engine(mode, **kw):
    prec, store, planes, _, _ = MODES[mode]
    return gpca.GpcaEngine(precision=prec, storage=store, digit_planes=planes, **kw)


def check_engine(e, G, mu, sigma, rows, ulps, l, nd, what, mask=None, row_slice=None):
    sc, sv, ld = e.scores(f64=True), e.singular_values(), e.loadings()
    if mask is not None:
        assert np.all(sc[~np.asarray(mask, bool)] == 0.0), what
    rr = rows if row_slice is None else rows[row_slice]
    uu = ulps if row_slice is None else ulps[row_slice]
    truth = k1_truth(G, mu, sigma, rr, sc, sv, mask)
    return check(ld, truth, k1_bar(G, mu, sigma, rr, sc, sv, l, nd, truth, mask, uu), what)


def run_rsvd_case(oracle, mode, M, N, k, os_, q, seed=None, **kw):
    G, mu, sigma, rows = case_inputs(oracle, M, N, 1000 * N + M if seed is None else seed)
    l = k + os_
    assert l <= min(len(rows), N)
    rr = 1.0 / sigma[rows].astype(np.float64)
    assert rr.max() / rr.min() >= min(30.0, np.sqrt(N) / 2), "r must span what the sample count allows (30 x from about 2k samples)"
    with open_engine(mode, **kw) as e:
        e.upload_genotypes_i8(G)
        ulps = device_stats(e, mu, sigma, rows)
        e.rsvd(k, os_, q, seed=7)
        return check_engine(e, G, mu, sigma, rows, ulps, l, MODES[mode][3], f"rsvd {mode} M={M} N={N} k={k}+{os_} q={q} {kw or ''}")


def small_sketch(oracle, M, N):
    """(k, oversample) for the rows x samples grid: (22, 10) where the kept rows allow it, else (5, 0)"""
    return (22, 10) if min(len(case_inputs(oracle, M, N, 1000 * N + M)[3]), N) >= 32 else (5, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("N", [64, 255, 256, 257, 1023, 1024, 1025, 2049])
@pytest.mark.parametrize("M", [31, 32, 33, 4097])
def test_rsvd_rows_and_samples(oracle, mode, M, N):
    k, os_ = small_sketch(oracle, M, N)
    run_rsvd_case(oracle, mode, M, N, k, os_, 2)
    if (k, os_) != (5, 0):
        run_rsvd_case(oracle, mode, M, N, 5, 0, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("q", [0, 2])
@pytest.mark.parametrize("mode,k,os_", [(m, k, o) for m in MODES for k, o in [(1, 0), (5, 0), (22, 10), (23, 10), (54, 10), (55, 10), (118, 10), (64, 0), (128, 0)]
                                        if k + o <= 64 or m in EXACT])      # (GPCA_PREC_F32_MFMA holds up to 64 sketch columns)
def test_rsvd_sketch_widths(oracle, mode, q, k, os_):
    """L = 32 / 64 / 128: one, two, four column halves ((64, 0), (128, 0): full halves with oversample 0, where the bar is tightest)"""
    run_rsvd_case(oracle, mode, 4097, 1025, k, os_, q)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["default", "simple", "gq_waves_8", "gq_waves_4_simple"])
@pytest.mark.parametrize("N", [256, 1025])
def test_rsvd_kernel_variants_int8(oracle, variant, N):
    """exact int8: k_gq_d / k_gq_n (N <= 256) by default, k_gq_i8 (GPCA_CFG_SIMPLE_KERNELS), GPCA_CFG_NO_NARROW on the narrow matrix, and small
    wave targets (multi-round sweeps, gq_chain) -- the truth is built once per shape and shared"""
    kw = {"default": {}, "simple": dict(flags=_lib.CFG_SIMPLE_KERNELS), "gq_waves_8": dict(gq_waves=8),
          "gq_waves_4_simple": dict(flags=_lib.CFG_SIMPLE_KERNELS, gq_waves=4)}[variant]
    for k, os_ in ((30, 0), (54, 10)):
        run_rsvd_case(oracle, "int8", 4097, N, k, os_, 2, **kw)
    if N <= 256:
        run_rsvd_case(oracle, "int8", 4097, N, 30, 0, 2, flags=kw.get("flags", 0) | _lib.CFG_NO_NARROW, gq_waves=kw.get("gq_waves", 0))
    for mode in ("2bit", "2bit4"):
        if variant in ("default", "gq_waves_8"):
            run_rsvd_case(oracle, mode, 4097, N, 30, 0, 2, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,simple", [(m, 0) for m in MODES] + [("int8", 1)])      # (GPCA_CFG_SIMPLE_KERNELS selects another K1 on int8 rows only)
@pytest.mark.parametrize("gq_waves", [8, 4])
def test_rsvd_row_group_remainders(oracle, mode, simple, gq_waves):
    """1790 rows = 56 units of 32: 8 waves own 7 units each (row groups of 4 + 2 + 1; 4 + 3 in k_gq_2bit), 4 waves own 14 (4 + 4 + 4 + 2):
    several rounds per wave and every remainder group of k_gq_i8, k_gq_d, k_gq_2bit and k_gq_f32"""
    M, N = 1790, 1025
    units = (M + 127) // 128 * 128 // 32                                       # (gq_plan, plan_math.h: the waves asked for are the waves used)
    assert units % gq_waves == 0 and units // gq_waves in (7, 14)
    run_rsvd_case(oracle, mode, M, N, 30, 0, 2, flags=_lib.CFG_SIMPLE_KERNELS if simple else 0, gq_waves=gq_waves)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", EXACT)
@pytest.mark.parametrize("fused", [True, False])
def test_rsvd_streamed_panels(oracle, mode, fused):
    """streamed, panel_rows (1024) does not divide M (4097: the last panel holds one row): per-panel row0 offsets of stage_AQ.  Exact modes only:
    rsvd_preflight refuses streamed panels on GPCA_PREC_F32_MFMA."""
    M, N = 4097, 1025
    G, mu, sigma, rows = case_inputs(oracle, M, N, 1000 * N + M)
    for k, os_ in ((30, 0), (54, 10)):
        with open_engine(mode) as e:
            e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), M, N, panel_rows=1024, ring_slots=2, fused=fused)
            ulps = device_stats(e, mu, sigma, rows)
            e.rsvd(k, os_, 2, seed=7)
            check_engine(e, G, mu, sigma, rows, ulps, k + os_, MODES[mode][3], f"streamed {mode} fused={fused} k={k}+{os_}")


@pytest.mark.gpu
@pytest.mark.parametrize("k,os_", [(30, 0), (22, 10)])
@pytest.mark.parametrize("mode", list(MODES))
def test_rsvd_two_row_shards_one_gpu(oracle, mode, k, os_):
    """two row shards on one GPU through the allreduce hook: each rank's loadings against its own rows, the scores and sv of all"""
    M, N = 4097, 1025
    G, mu, sigma, rows = case_inputs(oracle, M, N, 1000 * N + M)
    spans = [gpca.shard_rows(M, 2, r) for r in range(2)]
    barrier = threading.Barrier(2); bufs = [None, None]; res = [None, None]; errs = []

    def run(rank):
        try:
            a, b_ = spans[rank]
            with open_engine(mode) as e:
                e.upload_genotypes_i8(G[a:b_])
                mine = rows[(rows >= a) & (rows < b_)]
                ulps = device_stats(e, mu[a:b_], sigma[a:b_], mine - a)

                def hook(buf):
                    bufs[rank] = buf.copy(); barrier.wait()
                    buf[:] = bufs[0] + bufs[1]; barrier.wait()
                e.set_allreduce_hook(hook, 2, rank, a)
                e.rsvd(k, os_, 2, seed=7)
                res[rank] = (e.scores(f64=True), e.singular_values(), e.loadings(), mine, ulps)
        except BaseException as ex:  # noqa: BLE001 -- reported by the main thread
            errs.append(ex); barrier.abort()
    ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    [t.start() for t in ts]; [t.join() for t in ts]
    assert not errs, errs
    for rank in range(2):
        sc, sv, ld, mine, ulps = res[rank]
        truth = k1_truth(G, mu, sigma, mine, sc, sv)
        check(ld, truth, k1_bar(G, mu, sigma, mine, sc, sv, k + os_, MODES[mode][3], truth, None, ulps), f"two shards {mode} k={k}+{os_} rank {rank}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_rsvd_compact_child(oracle, mode):
    """QC keeps a fifth of 70 000 rows: the sweep runs on the gathered child (its own row numbering, r and b gathered)"""
    M, N = 70_000, 320
    G = make_genotypes(M, N, seed=9, drop=False)
    st = oracle.snp_stats(G, N, 0.0, 0.0, 1.0)
    keep = ((np.random.default_rng(0).random(M) < 0.2) & (st["keep"] != 0)).astype(np.uint8)
    mu, sigma, rows = st["mu"], st["sigma"], np.flatnonzero(keep)
    with open_engine(mode) as e:
        e.upload_genotypes_i8(G)
        dst = e.snp_stats(gpca.QcConfig.none())
        assert np.array_equal(dst["mu"][rows], mu[rows])
        ulps = np.abs(dst["sigma"][rows].astype(np.float64) - sigma[rows].astype(np.float64)) / np.spacing(sigma[rows]).astype(np.float64)
        assert np.all(ulps <= 1)
        e.set_standardization(mu, sigma, keep)                   # (the CPU's mu, sigma from here on)
        e.enable_timings(True)
        for k, os_ in ((30, 0), (22, 10)):
            e.reset_timings()
            e.rsvd(k, os_, 2, seed=7)
            tim = e.timings()
            per = 0.25 if MODES[mode][4] else 1.0
            assert abs(tim["gemm_GQ"]["bytes"] / tim["gemm_GQ"]["launches"] / (N * per) - len(rows)) < 1, "the call did not run on the compact child"
            check_engine(e, G, mu, sigma, rows, np.zeros(len(rows)), k + os_, MODES[mode][3], f"compact child {mode} k={k}+{os_}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_rsvd_with_a_sample_mask(oracle, mode):
    """gpca_set_sample_mask, then gpca_rsvd: the sum runs over the masked samples, sv are the subset's"""
    M, N = 4097, 1025
    G, mu, sigma, rows = case_inputs(oracle, M, N, 1000 * N + M)
    mask = (np.random.default_rng(4).random(N) < 0.6).astype(np.uint8)
    mask[-1] = 1
    for k, os_ in ((30, 0), (22, 10)):
        with open_engine(mode) as e:
            e.upload_genotypes_i8(G)
            ulps = device_stats(e, mu, sigma, rows)
            e.set_sample_mask(mask)
            e.rsvd(k, os_, 2, seed=7)
            check_engine(e, G, mu, sigma, rows, ulps, k + os_, MODES[mode][3], f"sample mask {mode} k={k}+{os_}", mask=mask)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("N", [257, 1025])
def test_refine(oracle, mode, N):
    """gpca_refine from S0 with non-zero column means: k = 1 element by element against A q / |A q|, k = 33 (two column halves) through the
    span of A Q"""
    M, nd = 4097, MODES[mode][3]
    G, mu, sigma, rows = case_inputs(oracle, M, N, 1000 * N + M)
    with open_engine(mode) as e:
        e.upload_genotypes_i8(G)
        device_stats(e, mu, sigma, rows)
        sg = e.get_standardization()["sigma"]
        e.set_standardization(mu, sigma, np.isin(np.arange(M), rows).astype(np.uint8))      # (the CPU's sigma: the bars below know Q, not 1-ulp slack)
        assert np.max(np.abs(sg[rows].astype(np.float64) - sigma[rows])) <= np.max(np.spacing(sigma[rows]))
        s0 = refine_start(N, 1, seed=N)
        e.refine(s0)
        ld = e.loadings().astype(np.float64)
        truth, bar = refine1_bar(G, mu, sigma, rows, s0[:, 0], nd)
        check(ld * np.sign(np.sum(ld * truth)), truth, bar, f"refine {mode} N={N} k=1")
        S0 = refine_start(N, 33, seed=N + 1)
        e.refine(S0)
        ld = e.loadings().astype(np.float64)
        Qb, rbar = refine_span_bar(G, mu, sigma, rows, S0, nd)
        check(ld - Qb @ (Qb.T @ ld), np.zeros_like(ld), np.repeat(rbar[:, None], 33, axis=1), f"refine {mode} N={N} k=33 (span residual)")
