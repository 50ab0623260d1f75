"""One pass of the exact-integer path, held to a bar derived from its own arithmetic (gemm_i8.hip, fold_quantize_i8.hip, project.hip).

Subjects: gpca_project with a caller's mu, sigma, W, and gpca_transform after a fit, on GPCA_PREC_I8_EXACT: int8 rows (4 digit planes),
2-bit rows (3 planes, the default) and 2-bit rows with digit_planes = 4.  Neither call corrects itself, so an error of one pass shows.

THE MODEL (``exact_pass_model``; written from DESIGN.md and the sources, never from device outputs).  Model rows = rows of W that are not
all zero.  In f32, as launch_set_scale and launch_scale_rows make them:  r_i = 1 / sigma_i,  b_i = -mu_i r_i,  Ta = r_i W_ij,
Tb = b_i W_ij.  Per column and side:  colmax = max_i |T_ij|,  q_ij = rint(T_ij * (S / colmax)) as an integer,  S = 0.49 * 128^4 (four
signed base-128 digits in [-64, 63], the top one the remainder) or 0.49 * 256^3 (three signed base-256 digits in [-128, 127]).
    Yint_a[n][j] = sum_i g'[i][n] qa_ij   (g' = the dosage, 0 for a missing call)       Yint_b[n][j] = sum_i [g[i][n] missing] qb_ij
    c_j = sum_i Tb_ij        Y[n][j] = (colmax_a / S) Yint_a + c_j - (colmax_b / S) Yint_b,    0 for a sample with no observed model row.

THE BAR AGAINST THE MODEL (``bounds``), per sample and column; the integer sums must agree exactly, what remains is
    f64:  u64 * (P + 2) * (|scale_a Yint_a| + |c_j| + |scale_b Yint_b| + sum_i |Tb_ij|)     u64 = 2^-53, P = ceil(Mpad / 64) partials of c
          (two fused multiply-adds of the recombination and the f64 fold of c's P partials; the model itself recombines in long double)
    f32:  u32 * 64 * sum_i |Tb_ij|                                                           u32 = 2^-24, 64 rows per f32 partial of c
    ties: an entry of T * (S / colmax) within 4 ulp of a half-integer may round either way: count_j * colmax_j / S (counted on the CPU; the
          seeded inputs leave the count at 0 in at least 95 % of the columns, checked before anything is launched).
THE BAR AGAINST THE TRUTH (ref_project, f64): the quantisation, 0.5 (colmax_a / S) sum_i |g'[i][n]| + 0.5 (colmax_b / S) (missing model
rows of n), plus the terms above.  That is the whole error when r and Ta are exact in f32: the ``pow2`` inputs take sigma from
{1, 1/2, .., 1/32} (r spans 32 x within every column).  For any other sigma (``generic`` inputs, the fitted model of gpca_transform) r,
b, Ta and Tb are each rounded to f32 once, which the truth does not do, and the bar adds  u32 * (2 sum_i |g' Ta_ij| + 3 sum_i |Tb_ij|).
No constant is picked by hand: every term is a formula over the test's inputs.

TEETH (CPU, no GPU mark): six mutations of the model -- lowest digit plane dropped, digit base off by one, last 32-row unit left out of
the integer sum, last 64-row group left out of c, colmax over the first half of the rows only (the digits then wrap as int8 does),
missing calls counted as dosage 3 -- must each break the bar against the model on the test's own inputs.  mu is small (0.002 .. 0.02)
in these inputs: the f32 term of the bar is proportional to sum |b W| = sum mu |r W|, and with mu of order one it would hide the lowest
plane of a four-plane operand.

Measured on one MI355X, the largest fraction of a bar over every case, sample and column (each test prints its own with -s):
    gpca_project    against the model 0.022 (all three modes);  against ref_project 0.30 (int8), 0.55 (2-bit, 3 planes), 0.30 (2-bit, 4 planes)
    gpca_transform  against the model 0.0011 / 0.0010 / 0.0011;  against ref_project 0.0094 / 0.059 / 0.0094"""
import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib

U64, U32 = 2.0 ** -53, 2.0 ** -24
MISSING = -127
# storage mode -> (storage, digit_planes argument, planes in use)
MODES = {"int8": (_lib.STORE_INT8, 0, 4), "2bit": (_lib.STORE_2BIT, 0, 3), "2bit4": (_lib.STORE_2BIT, 4, 4)}


def digit_scale(nd):
    return 0.49 * 256.0 ** 3 if nd == 3 else 0.49 * 128.0 ** 4


def split_digits(q, nd, wrap=False):
    """The signed digits of q (int64 array), least significant first, as split_digits of fold_quantize_i8.hip makes them; wrap: the top
    digit is stored in a signed byte (what the planes hold when q is larger than the scale allows)."""
    base, half = (256, 128) if nd == 3 else (128, 64)
    v = q.astype(np.int64).copy()
    out = []
    for d in range(nd):
        if d < nd - 1:
            dg = ((v + half) & (base - 1)) - half
            v = (v - dg) // base
        else:
            dg = ((v + 128) & 255) - 128 if wrap else v
        out.append(dg)
    return out, base


def scale_f32(mu, sigma, W):
    """r, b, Ta, Tb in f32 as launch_set_scale / launch_scale_rows make them (0 on rows outside the model)"""
    mu, sigma, W = np.asarray(mu, np.float32), np.asarray(sigma, np.float32), np.asarray(W, np.float32)
    model = np.any(W != 0, axis=1)
    ok = model & ~(np.abs(sigma) < np.float32(1e-9))
    r = np.where(ok, np.float32(1) / np.where(ok, sigma, np.float32(1)), np.float32(0)).astype(np.float32)
    b = np.where(ok, (-mu * r).astype(np.float32), np.float32(0)).astype(np.float32)
    return model, r, b, (r[:, None] * W).astype(np.float32), (b[:, None] * W).astype(np.float32)


def quantize(T, nd, rows_for_max=None):
    """(q int64, scale = colmax / S, ties per column) of one side"""
    S = digit_scale(nd)
    Td = T.astype(np.float64)
    colmax = np.max(np.abs(Td if rows_for_max is None else Td[:rows_for_max]), axis=0) if T.shape[0] else np.zeros(T.shape[1])
    with np.errstate(divide="ignore"):
        inv = np.where(colmax > 0, S / np.where(colmax > 0, colmax, 1.0), 0.0)
        scale = np.where(colmax > 0, colmax / S, 0.0)
    t = Td * inv[None, :]
    q = np.rint(t).astype(np.int64)
    ties = np.sum(np.abs(np.abs(t - np.floor(t)) - 0.5) <= 4 * np.spacing(np.abs(t)), axis=0)
    return q, scale, ties


def int_dot(A, q):
    """A^T q exactly (A small integers [M][N], q int64 [M][k]): every partial sum is an integer below 2^53, so the f64 product is exact"""
    assert float(np.max(np.abs(A), initial=0)) * float(np.max(np.abs(q), initial=0)) * max(A.shape[0], 1) < 2.0 ** 53
    return (A.astype(np.float64).T @ q.astype(np.float64)).astype(np.int64)


def exact_pass_model(G, mu, sigma, W, nd, mutate=None):
    """The fixed-point model of one gpca_project pass (gpca_transform: the same with no missing call).  Returns a dict with Y (long double
    recombination, as f64), the per-(sample, column) bars and what they are made of."""
    G = np.asarray(G, np.int8)
    M, N = G.shape
    model, r, b, Ta, Tb = scale_f32(mu, sigma, W)
    miss = (G == MISSING) & model[:, None]
    ga = np.where(G == MISSING, 3 if mutate == "missing_as_3" else 0, G).astype(np.int64)
    half_rows = (M + 1) // 2 if mutate == "colmax_first_half" else None
    qa, sa, ties_a = quantize(Ta, nd, half_rows)
    qb, sb, ties_b = quantize(Tb, nd, half_rows)
    digits_ok = True
    if mutate is None:                                        # the model's own digits fit the range the kernel header states
        lim = (128, 127) if nd == 3 else (64, 63)
        for q in (qa, qb):
            dg, base = split_digits(q, nd)
            digits_ok &= all(int(d.min(initial=0)) >= -lim[0] and int(d.max(initial=0)) <= lim[1] for d in dg)
            assert np.array_equal(sum(d * base ** i for i, d in enumerate(dg)), q)
        Yia, Yib = int_dot(ga, qa), int_dot(miss.astype(np.int64), qb)
    else:
        sides = []
        for A, q in ((ga, qa), (miss.astype(np.int64), qb)):
            dg, base = split_digits(q, nd, wrap=True)
            if mutate == "drop_lowest_plane":
                dg[0] = np.zeros_like(dg[0])
            if mutate == "last_unit_out":
                A = A.copy(); A[(M - 1) // 32 * 32:] = 0
            wbase = base - 1 if mutate == "base_off_by_one" else base
            sides.append(sum(int_dot(A, d) * wbase ** i for i, d in enumerate(dg)))
        Yia, Yib = sides
    ld = np.longdouble
    Tb_c = Tb[:(M - 1) // 64 * 64] if mutate == "last_group_out_of_c" else Tb
    c = np.sum(Tb_c.astype(ld), axis=0)
    Y = (sa.astype(ld)[None, :] * Yia.astype(ld) + c[None, :]) - sb.astype(ld)[None, :] * Yib.astype(ld)
    n_model = int(model.sum())
    cnt = miss.sum(axis=0)
    Y[cnt == n_model] = 0
    return dict(Y=Y.astype(np.float64), c=c.astype(np.float64), sa=sa, sb=sb, Yia=Yia, Yib=Yib, Ta=Ta, Tb=Tb, ties_a=ties_a, ties_b=ties_b,
                ga=np.where(G == MISSING, 0, G).astype(np.float64) * model[:, None], miss=miss, used=(n_model - cnt).astype(np.int32),
                digits_ok=digits_ok, M=M)


def bounds(m, generic):
    """(bar against the model, bar against ref_project), both [N][k]: the module docstring's formulas"""
    sum_tb = np.sum(np.abs(m["Tb"].astype(np.float64)), axis=0)
    P = (((m["M"] + 127) // 128 * 128) + 63) // 64
    t1 = np.abs(m["sa"][None, :] * m["Yia"]) + np.abs(m["c"])[None, :] + np.abs(m["sb"][None, :] * m["Yib"])
    f64 = U64 * (P + 2) * (t1 + sum_tb[None, :])
    f32 = U32 * 64 * sum_tb
    ties = m["ties_a"] * m["sa"] + m["ties_b"] * m["sb"]
    bar_model = f64 + (f32 + ties)[None, :]
    quant = 0.5 * (np.sum(m["ga"], axis=0)[:, None] * m["sa"][None, :] + np.sum(m["miss"], axis=0)[:, None] * m["sb"][None, :])
    bar_truth = bar_model + quant
    if generic:
        bar_truth = bar_truth + U32 * (2 * (m["ga"].T @ np.abs(m["Ta"].astype(np.float64))) + 3 * sum_tb[None, :])
    return bar_model, bar_truth


def ref_project(G, mu, sigma, W):
    """the truth in f64 (tests/test_gpu_project.py: the same function)"""
    model = np.any(W != 0, axis=1)
    obs = (G != MISSING) & model[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):      # (rows outside the model may have sigma = 0: masked)
        Z = np.where(obs, (G.astype(np.float64) - mu.astype(np.float64)[:, None]) / sigma.astype(np.float64)[:, None], 0.0)
    return Z.T @ W.astype(np.float64), obs.sum(axis=0).astype(np.int32)


def make_inputs(M, N, k, miss, family, seed):
    """Genotypes and a model with the places where an exact pass goes wrong: r = 1 / sigma spans 32 x (pow2: sigma in {1 .. 1/32}; generic:
    log-uniform on [1/32, 1]) inside every column; column 0's maximum sits in row 0, column k - 1's in the very last row (four times the
    rest, with the largest r); column k // 2 is all zero (k >= 3); a sample with every call missing where miss > 0 (and N > 1)."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.5, size=(M, 1))
    G = (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)
    if miss > 0:
        G[rng.random((M, N)) < miss] = MISSING
        if N > 1:
            G[:, N // 2] = MISSING
    if family == "pow2":
        sigma = (2.0 ** -rng.integers(0, 6, M)).astype(np.float32)
    else:
        sigma = np.exp(rng.uniform(np.log(1 / 32), 0.0, M)).astype(np.float32)
    mu = rng.uniform(0.002, 0.02, M).astype(np.float32)
    W = (rng.standard_normal((M, k)) * 0.05).astype(np.float32)
    W[np.abs(W) < 1e-4] = np.float32(1e-4)                   # (every row a model row)
    top = np.float32(4 * np.max(np.abs(W)))
    sigma[0] = sigma[M - 1] = np.float32(1 / 32)
    W[0, 0] = top
    W[M - 1, k - 1] = -top
    if k >= 3:
        W[:, k // 2] = 0
    return G, mu, sigma, W


def few_ties(m):
    t = np.concatenate([m["ties_a"], m["ties_b"]])
    return np.mean(t == 0) >= 0.95


# ---- teeth: every mutation of the model must break the bar against the model, on the test's own inputs (CPU only) -------------------------
MUTATIONS = ["drop_lowest_plane", "base_off_by_one", "last_unit_out", "last_group_out_of_c", "colmax_first_half", "missing_as_3"]


@pytest.mark.parametrize("family", ["pow2", "generic"])
@pytest.mark.parametrize("M", [33, 4097])
@pytest.mark.parametrize("nd", [3, 4])
def test_the_bar_rejects_every_mutant(nd, M, family):
    N, k = 257, 33
    G, mu, sigma, W = make_inputs(M, N, k, 0.01, family, seed=M + nd)
    m = exact_pass_model(G, mu, sigma, W, nd)
    assert m["digits_ok"] and few_ties(m)
    bar, _ = bounds(m, family == "generic")
    for mut in MUTATIONS:
        y = exact_pass_model(G, mu, sigma, W, nd, mutate=mut)["Y"]
        worst = float(np.max(np.abs(y - m["Y"]) / np.where(bar > 0, bar, np.inf)))
        print(f"nd={nd} M={M} {family}: mutant {mut}: max |dY| / bar = {worst:.3g}")
        assert np.any(np.abs(y - m["Y"]) > bar), f"the bar lets the mutant '{mut}' through"


def test_the_model_agrees_with_the_truth_within_its_own_bar():
    """the model against ref_project on the CPU: the quantisation bound is a bound"""
    for nd in (3, 4):
        for family in ("pow2", "generic"):
            G, mu, sigma, W = make_inputs(4097, 129, 33, 0.01, family, seed=nd)
            m = exact_pass_model(G, mu, sigma, W, nd)
            bar_model, bar_truth = bounds(m, family == "generic")
            ref, used = ref_project(G, mu, sigma, W)
            assert np.all(np.abs(m["Y"] - ref) <= bar_truth) and np.array_equal(m["used"], used)


# ---- the device ------------------------------------------------------------------------------------------------------------------------------
def check_against_bars(sc, G, mu, sigma, W, nd, generic, what):
    """every sample and every column of a device result against both bars; returns the two worst fractions of a bar"""
    m = exact_pass_model(G, mu, sigma, W, nd)
    bar_model, bar_truth = bounds(m, generic)
    ref, _ = ref_project(np.asarray(G), np.asarray(mu, np.float32), np.asarray(sigma, np.float32), np.asarray(W, np.float32))
    assert np.all(np.isfinite(sc)), what
    d_model, d_truth = np.abs(sc - m["Y"]), np.abs(sc - ref)
    fm = float(np.max(np.where(bar_model > 0, d_model / np.where(bar_model > 0, bar_model, 1), np.where(d_model > 0, np.inf, 0)), initial=0))
    ft = float(np.max(np.where(bar_truth > 0, d_truth / np.where(bar_truth > 0, bar_truth, 1), np.where(d_truth > 0, np.inf, 0)), initial=0))
    print(f"{what}: max |Y_device - Y_model| / bar = {fm:.3g}, max |Y_device - Y_truth| / bar = {ft:.3g}")
    assert np.all(d_model <= bar_model), f"{what}: {fm:.3g} of the bar against the model"
    assert np.all(d_truth <= bar_truth), f"{what}: {ft:.3g} of the bar against ref_project"
    return m, fm, ft


def run_project_case(mode, M, N, k, miss, seed):
    store, planes, nd = MODES[mode]
    cases = []
    for family in ("pow2", "generic"):
        G, mu, sigma, W = make_inputs(M, N, k, miss, family, seed)
        m = exact_pass_model(G, mu, sigma, W, nd)
        assert m["digits_ok"], "the model's own digits leave the range the kernel states"
        cases.append((family, G, mu, sigma, W, m))
    assert all(few_ties(c[5]) for c in cases)                            # (checked before anything is launched)
    for family, G, mu, sigma, W, m in cases:
        with gpca.GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=store, digit_planes=planes) as e:
            e.upload_genotypes_i8(G)
            sc, used = e.project(mu, sigma, W)
        what = f"project {mode} M={M} N={N} k={k} miss={miss} {family}"
        check_against_bars(sc, G, mu, sigma, W, nd, family == "generic", what)
        assert np.array_equal(used, m["used"]), what
        if k >= 3:
            assert np.all(sc[:, k // 2] == 0.0), what + ": an all-zero column of W must give exactly c_j = 0"
        if miss > 0 and N > 1:
            assert np.all(sc[N // 2] == 0.0) and used[N // 2] == 0, what


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1023, 1024, 1025])
@pytest.mark.parametrize("M", [31, 32, 33, 4097])
def test_project_rows_and_samples(mode, M, N):
    run_project_case(mode, M, N, 33, 0.01, seed=1000 * N + M)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("miss", [0.0, 0.01])
@pytest.mark.parametrize("k", [1, 32, 33, 64, 65, 128])
def test_project_columns_and_missing_rates(mode, k, miss):
    run_project_case(mode, 4097, 257, k, miss, seed=7 * k + int(miss * 100))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("k", [1, 33])
def test_transform_after_a_fit(mode, k):
    """gpca_transform on the fitted matrix: one pass with the handle's own mu, sigma and loadings (no missing call)"""
    store, planes, nd = MODES[mode]
    M, N = 4097, 2049
    rng = np.random.default_rng(k)
    p = np.exp(rng.uniform(np.log(0.0003), np.log(0.5), size=(M, 1)))        # singletons next to common variants: r spans over 30 x
    G = (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)
    with gpca.GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=store, digit_planes=planes) as e:
        e.upload_genotypes_i8(G)
        e.snp_stats(gpca.QcConfig.none())
        e.rsvd(k, 10, 2, seed=3)
        tr = e.transform()
        st = e.get_standardization()
        W = np.zeros((M, k), np.float32)
        W[e.pca_snp_rows()] = e.loadings()
    kept = np.flatnonzero(np.any(W != 0, axis=1))
    rr = 1.0 / st["sigma"][kept].astype(np.float64)
    assert rr.max() / rr.min() >= 30
    check_against_bars(tr, G, st["mu"], st["sigma"], W, nd, True, f"transform {mode} k={k}")
