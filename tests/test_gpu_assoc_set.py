"""gpca_assoc_logistic_set: the covariance of the scores inside a set (assoc_set.hip, gpca_assoc_score.cpp), through the C ABI, and the
set tests made from it (gpca_set_test).

The definitions (include/gpca.h section a16), restated in numpy f64 (``phi_restate``).  The setting is that of
tests/test_gpu_assoc_score.py, whose ``panel`` and ``restate`` this module uses: the operand x (g, or 2 - g on a flipped row), m =
[missing and in S], xbar the operand's mean, w the panel's column 1.  Per pair of rows of a set and per trait
    XX = sum x_a x_b w,  XM = sum x_a m_b w,  MX = sum m_a x_b w,  MM = sum m_a m_b w
    R = (XX + (xbar_b XM + xbar_a MX)) + (xbar_a xbar_b) MM,   Phi^op = (R - a_a,0 a_b,0) - sum_{j >= 1} a_a,j a_b,j,   Phi = s_a s_b Phi^op
with the a of the DEVICE's own ua, so that the bar below is the Gram kernel's and its epilogue's alone.

The bar (u = 2^-24, e = 2^-53, F = 256 = kAscFlush).  Every term of the four sums is non-negative, and so is xbar, so R is its own sum of
absolute values.
  f32 side: w rounds once to f32 (u; w x_b and w m_b are then exact, and so is every product); every partial sum of a flush group of at
    most F terms rounds once, and a v_mfma_f32_32x32x2_f32 that rounds the sum of its two products costs one more: (F + 3) u R covers
    the first order F + 2 and the second, as for the score scan.
  f64 side, counted along the longest path of a term into R: N / F + 1 additions of flush groups, the division that makes xbar (two of
    them meet in the MM term, one more), the product with xbar (two in the MM term), and three additions: N / F + 1 + 2 + 2 + 3 - 2 =
    N / F + 6 roundings at most, each relative to a partial result below R: (N / F + 6) e R.
  epilogue: 1 + Pc products, each rounded once, Pc - 1 additions inside q and two subtractions, every partial result at most
    R + sum_j |a_a,j a_b,j| in magnitude: at most (2 Pc + 2) e (R + sum |a_a a_b|) on the device, the same again in this module's numpy
    (which sums in another order); 4 (Pc + 3) e (R + sum |a_a a_b|) covers both.
      bar = ((F + 3) u + (N / F + 6) e) R + 4 (Pc + 3) e (R + sum_j |a_a,j a_b,j|)
  (F + 3) u N < 1 / 2 at N = 1 025 (asserted): the bar stays under half an average term, and every shape asserts that leaving one
  included sample out of the restatement breaks it somewhere.
End to end against g~_a^T W g~_b formed directly in f64 in A1 coding (``direct_phi``): Phi = G~ W G~^T - (G~ W X)(X^T W X)^-1 (X^T W G~),
  first order from the ua bars of tests/test_gpu_assoc_score.py: d Phi_ab = d R_ab + sum_j (|a_a,j| d a_b,j + |a_b,j| d a_a,j), doubled
  for the second order, plus the formula's own error (64 kappa^2 + N) e sqrt((g~_a^T W g~_a)(g~_b^T W g~_b)): the solve with X^T W X,
  and numpy's sums of N products (the two terms cancel entirely on a monomorphic row, where nothing else is left).
Every case prints the largest fraction of the bar it observes ("phi: max err / bar").

What it is for (test_set_tests_on_a_cohort): N = 2 000, 10 % cases (logit P = alpha + sum_j beta_j (g_j - mean), alpha solved for the
rate), one set of 20 variants, heterozygous carriers at random samples: 5 at MAF 0.7 - 1 % (28 - 39 carriers; the causal ones) and 15
with one carrier each, Beta(maf; 1, 25) weights.
  mixed:  beta = (1.5, -3, 1.5, -3, 1.5)   bound SKAT - burden >= 2 decades
  same:   beta = 0.8 each                   bound burden - SKAT >= 0.5 decades
  null:   beta = 0                          bound both -log10 p < 2
Seed 2, chosen among seeds 1 .. 12 as the first where the f64 restatement alone (``cohort_restatement``: the engine's null fit, the
direct Phi, this repository's numpy restatement of the rule) clears each bound by a factor of at least 2:
  mixed: SKAT 10.62, burden 5.46 (5.16 >= 2 x 2);  same: burden 5.75, SKAT 3.14 (2.61 >= 2 x 0.5);  null: SKAT 0.68, burden 0.56 (< 2 / 2).
The device is asserted at the bounds."""
import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from genomic_pca_amd._lib import GpcaError

from test_assoc_set_host import set_test_reference
from test_gpu_assoc_score import STORES, VIF, design, load, null_mu, panel, restate, same

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS = 2.0 ** -53
F_ASC = 256           # kAscFlush (plan_math.h)
assert (F_ASC + 3) * U * 1025 < 0.5
K_ROWS = 300
NS = [4, 63, 64, 65, 255, 256, 257, 1025]
MS = [127, 2, 1, 33, 128, 31, 32, 64, 65]          # in list order: the 2-row set lies at list positions 127 and 128, the 1-row set at 129
assert sorted(MS) == [1, 2, 31, 32, 33, 64, 65, 127, 128]
TPS = [(1, 0), (2, 29), (16, 1), (1, 61)]
ROW_FLIP, ROW_MONO, ROW_TIE, ROW_A, ROW_B, ROW_NONE = 0, 2, 3, 5, 6, K_ROWS // 2
SPECIAL = [ROW_FLIP, ROW_MONO, ROW_TIE, ROW_A, ROW_B, ROW_NONE]
COHORT_SEED = 2      # module docstring


# ------------------------------------------------------------------------------------------------ inputs
def make_set_inputs(N, T, Pc, seed):
    """K_ROWS rows x N samples of two populations, 3 % of the calls missing; about one sample in ten excluded (the excluded samples
    hold missing calls and extreme trait and covariate values); sample N // 3 (included) has every call missing.  All of this from 16
    samples on: the 4-sample shape needs its four samples for the null fit (two cases, two controls) and for a row to keep a
    variance, so it runs with everyone included and random rows only.  ROW_FLIP has an A1 frequency of 0.9 (it flips), ROW_MONO is monomorphic among the included samples, ROW_TIE has
    s1 = n_obs exactly (it does not flip), ROW_NONE has no observed call, and ROW_A / ROW_B have a missing call at an included sample in
    A only, at another in B only and at a third in both."""
    rng = np.random.default_rng(seed)
    pop = np.arange(N) % 2
    p = np.stack([rng.uniform(0.1, 0.9, K_ROWS), rng.uniform(0.1, 0.9, K_ROWS)], 1)[:, pop]
    G = (rng.random((K_ROWS, N)) < p).astype(np.int8) + (rng.random((K_ROWS, N)) < p).astype(np.int8)
    inc = np.ones(N, np.uint8)
    if N >= 16:
        inc[rng.random(N) < 0.1] = 0
        inc[N // 3] = 1
    G[rng.random((K_ROWS, N)) < 0.03] = -127
    G[:, inc == 0] = -127
    if N >= 8:
        G[:, N // 3] = -127
    C = rng.standard_normal((N, Pc))
    n = np.arange(N)
    Y = (rng.random((N, T)) < 1.0 / (1.0 + np.exp(-(0.8 * (n % 2) - 0.4)))[:, None]).astype(np.float64)
    if N == 4:
        Y[:] = np.array([0.0, 1.0, 0.0, 1.0])[:, None]
    s = inc == 1
    special = N >= 16
    if special:
        o0 = np.flatnonzero(s & (G[ROW_FLIP] != -127))
        G[ROW_FLIP, o0] = np.where(np.arange(len(o0)) % 5 == 0, 1, 2)
        G[ROW_NONE, :] = -127
        G[ROW_MONO, s & (G[ROW_MONO] != -127)] = 2
        o = np.flatnonzero(s & (G[ROW_TIE] != -127))
        G[ROW_TIE, o] = np.where(np.arange(len(o)) % 2 == 0, 0, 2)
        if len(o) % 2:
            G[ROW_TIE, o[-1]] = 1
        free = [int(i) for i in np.flatnonzero(s) if i != N // 3][:3]
        G[ROW_A, free] = [-127, 1, -127]
        G[ROW_B, free] = [2, -127, -127]
    Y[inc == 0] = 1e30
    C[inc == 0] = -1e30
    return G, Y, C, inc, special


def make_sets(seed):
    """the sets of a call, in the order of MS: sorted random rows of the K_ROWS (far apart); the 2-row set is (ROW_A, ROW_B), the 33-row
    and the 128-row set hold every special row (and with them that pair, at other positions)"""
    rng = np.random.default_rng(seed)
    sets = []
    for m in MS:
        if m == 2:
            rows = [ROW_A, ROW_B]
        elif m in (33, 128):
            rest = [r for r in rng.permutation(K_ROWS) if r not in SPECIAL][: m - len(SPECIAL)]
            rows = sorted(SPECIAL + [int(r) for r in rest])
        else:
            rows = sorted(int(r) for r in rng.choice(K_ROWS, m, replace=False))
        sets.append(np.array(rows, np.int64))
    return sets


# ------------------------------------------------------------------------------------------------ the f64 restatement
def phi_restate(Gs, Bs, inc, ua, Pc, drop=None):
    """Phi [T][m][m] of the rows Gs [m][N] of one set with the device's ua [m][T][Pc + 3], and its bar; drop: an included sample left
    out of the four sums"""
    s = np.asarray(inc).astype(bool)
    m, N = Gs.shape
    o = (Gs != -127) & s
    ms = ((Gs == -127) & s).astype(np.float64)
    g = np.where(o, Gs, 0).astype(np.float64)
    nobs, s1 = o.sum(1), g.sum(1)
    flip = s1 > nobs
    x = np.where(o, np.where(flip[:, None], 2.0 - g, g), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        xbar = np.where(flip, 2.0 * nobs - s1, s1) / nobs
    sg = np.where(flip, -1.0, 1.0)
    f = (F_ASC + 3) * U + (N / F_ASC + 6) * EPS
    phi, bar = np.zeros((len(Bs), m, m)), np.zeros((len(Bs), m, m))
    for t, B in enumerate(Bs):
        w = B[:, 1].copy()
        if drop is not None:
            w[drop] = 0.0
        with np.errstate(invalid="ignore"):
            XX, XM, MX, MM = (x * w) @ x.T, (x * w) @ ms.T, (ms * w) @ x.T, (ms * w) @ ms.T
            R = (XX + (xbar[None, :] * XM + xbar[:, None] * MX)) + (xbar[:, None] * xbar[None, :]) * MM
            a = ua[:, t, 2:]
            phi[t] = np.outer(sg, sg) * (R - a @ a.T)
            bar[t] = f * R + 4 * (Pc + 3) * EPS * (R + np.abs(a) @ np.abs(a).T)
    return phi, bar


def direct_phi(Gs, C, inc, mu, t):
    """(Phi [m][m], the diagonal of G~ W G~^T, kappa) for trait t by the direct f64 formula in A1 coding; rows without an observed call
    give NaN"""
    s = np.asarray(inc).astype(bool)
    X = design(C, inc)
    w = mu[s, t] * (1.0 - mu[s, t])
    H = X.T @ (w[:, None] * X)
    g = Gs[:, s].astype(np.float64)
    ob = g != -127
    with np.errstate(all="ignore"):
        mean = np.where(ob, g, 0).sum(1) / ob.sum(1)
    gt = np.where(ob, g, mean[:, None])
    b = (gt * w) @ X
    big = (gt * w) @ gt.T
    return big - b @ np.linalg.solve(H, b.T), np.diag(big), np.linalg.cond(H)


# ------------------------------------------------------------------------------------------------ the edge shapes
def _cases():
    out = [(N, TPS[i % 4], i) for i, N in enumerate(NS[:-1])]
    return out + [(1025, tp, len(NS) - 1 + j) for j, tp in enumerate(TPS)]


_CASES = _cases()
_REF = {}


def _shape(N, tp):
    return tp[0], min(tp[1], N // 8)                   # Pc <= N / 8 is kept


assert {N for N, _, _ in _CASES} == set(NS) and {_shape(N, tp) for N, tp, _ in _CASES} >= set(TPS)     # every shape of the issue


@pytest.mark.parametrize("N,tp,i", _CASES)
def test_sets_at_edge_shapes(N, tp, i):
    """every assertion of _check_case on int8 and on 2-bit storage, and the two storages' Phi bit for bit"""
    a, b = _check_case("int8", N, tp, i), _check_case("2bit", N, tp, i)
    assert len(a) == len(b) == len(MS) and all(same(x, y) for x, y in zip(a, b))


def _check_case(store, N, tp, i):
    T, Pc = _shape(N, tp)
    G, Y, C, inc, special = make_set_inputs(N, T, Pc, seed=900 + i)
    sets = make_sets(40 + i)
    listed = np.concatenate(sets)
    s = inc.astype(bool)
    if i not in _REF:
        mu = null_mu(Y, C, inc)
        Bs, kappas = panel(Y, C, inc, mu)
        drop = int(np.flatnonzero(s)[np.argmax(((G[:, s] != -127) & (G[:, s] != 0)).sum(0))])
        _REF[i] = (mu, Bs, kappas, restate(G, Bs, kappas, inc, Pc), drop)
    mu, Bs, kappas, ref, drop = _REF[i]
    if special:                                        # the rows the issue names are in the inputs, and inside sets
        assert ref["flip"][ROW_FLIP] and ref["s1"][ROW_TIE] == ref["nobs"][ROW_TIE] > 0 and not ref["flip"][ROW_TIE]
        assert ref["nobs"][ROW_NONE] == 0 and ref["nobs"][ROW_MONO] > 0
        assert ref["s2"][ROW_MONO] * ref["nobs"][ROW_MONO] == ref["s1"][ROW_MONO] ** 2
        assert s[N // 3] and np.all(G[:, N // 3] == -127)
        ma, mb = (G[ROW_A] == -127) & s, (G[ROW_B] == -127) & s
        assert (ma & ~mb).any() and (mb & ~ma).any() and (ma & mb).sum() >= 2
        for big in (3, 4):
            assert set(SPECIAL) <= set(sets[big].tolist())
    off = np.concatenate([[0], np.cumsum(MS)])
    assert off[1] == 127 and off[2] == 129 and off[3] == 130          # the list positions 127 / 128 / 129 are straddled
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        load(e, G)
        full = e.assoc_logistic_score(Y, C, include=inc, max_vif=VIF, ua=True)
        r = e.assoc_logistic_set(Y, sets, C, include=inc, max_vif=VIF, ua=True)
        alone = e.assoc_logistic_set(Y, [sets[1]], C, include=inc, max_vif=VIF)
    assert np.array_equal(r["set_off"], off) and len(r["phi"]) == len(MS)
    # 1. the listed rows carry the score scan's bits
    for k in ("beta", "se", "z", "vw", "V", "n_obs", "a1_freq", "xx", "flipped", "ua"):
        assert same(r[k], full[k][listed]), k
    worst = 0.0
    for si, rows in enumerate(sets):
        m = len(rows)
        lo, phi = int(off[si]), r["phi"][si]
        assert phi.shape == (T, m, m) and same(phi, np.transpose(phi, (0, 2, 1)))
        # 2. the diagonal carries V's bits
        assert same(np.diagonal(phi, axis1=1, axis2=2).T, r["V"][lo:lo + m]), si
        # 3. the derived bar, against the restatement formed from the device's own ua
        ua = r["ua"][lo:lo + m]
        want, bar = phi_restate(G[rows], Bs, inc, ua, Pc)
        dead = ref["nobs"][rows] == 0
        nanpat = dead[:, None] | dead[None, :]
        assert same(np.isnan(phi), np.broadcast_to(nanpat, phi.shape)) and same(np.isnan(want), np.isnan(phi)), si
        ok = ~np.isnan(want)
        err = np.abs(phi - want)
        assert np.all(err[ok] <= bar[ok]), (si, float(np.max(err[ok] / np.maximum(bar[ok], 1e-300))))
        if ok.any():
            worst = max(worst, float(np.max(err[ok] / np.maximum(bar[ok], 1e-300))))
        if m >= 31:
            dropped, _ = phi_restate(G[rows], Bs, inc, ua, Pc, drop=drop)
            assert np.any(np.abs(phi - dropped)[ok] > bar[ok]), si
        # 4. end to end: the direct formula in A1 coding, with the propagated ua bars
        ub = ref["bar"][rows]
        live = np.flatnonzero(~dead)
        for t in sorted({0, T - 1}):
            d, big, kap = direct_phi(G[rows], C, inc, mu, t)
            a, da = np.abs(ua[:, t, 2:]), ub[:, t, 2:]
            dphi = 2 * (bar[t] + a @ da.T + da @ a.T) + (64 * kap ** 2 + N) * EPS * np.sqrt(np.outer(big, big))
            sub = np.ix_(live, live)
            assert np.all(np.abs(phi[t][sub] - d[sub]) <= dphi[sub]), (si, t)
            # 6. positive semi-definite inside the bar
            if len(live):
                assert np.linalg.eigvalsh(phi[t][sub]).min() >= -np.linalg.norm(dphi[sub]), (si, t)
    print(store, "phi: max err / bar", worst, "kappa", max(kappas))
    # 5. a pair's bits do not depend on its set, its position or the call's other sets ...
    pair = r["phi"][1][:, 1, 0]
    for big in (3, 4):
        ia, ib = (int(np.flatnonzero(sets[big] == q)[0]) for q in (ROW_A, ROW_B))
        assert (ia, ib) != (0, 1) and same(r["phi"][big][:, ib, ia], pair), big
    assert same(alone["phi"][0], r["phi"][1])
    return r["phi"]                                    # (... nor on the storage: the caller compares)


@pytest.mark.parametrize("store", ["int8", "2bit"])
@pytest.mark.parametrize("N", [65, 257])
def test_recoding_the_alleles_keeps_phi(store, N):
    """a matrix and its 2 - g recoding (missing calls kept): every row's flip turns over (a tie stays unflipped in both), so the
    operands are the same and Phi in A1 coding, whose two signs both turn over, agrees inside the sum of the two propagated bars"""
    T, Pc = 2, 3
    G, Y, C, inc, special = make_set_inputs(N, T, Pc, seed=77)
    G2 = np.where(G == -127, G, 2 - G).astype(np.int8)
    sets = make_sets(5)[3:5]
    mu = null_mu(Y, C, inc)
    Bs, kappas = panel(Y, C, inc, mu)
    out = []
    for M in (G, G2):
        with gpca.GpcaEngine(storage=STORES[store]) as e:
            load(e, M)
            out.append((e.assoc_logistic_set(Y, sets, C, include=inc, max_vif=VIF, ua=True), restate(M, Bs, kappas, inc, Pc)["bar"]))
    (a, uba), (b, ubb) = out
    tie = a["flipped"] == b["flipped"]
    assert tie[list(np.concatenate(sets)).index(ROW_TIE)] and tie.sum() < 0.2 * len(tie)
    off = a["set_off"]
    for si, rows in enumerate(sets):
        m = len(rows)
        bars = []
        for M, r, ub in ((G, a, uba), (G2, b, ubb)):
            ua = r["ua"][off[si]:off[si] + m]
            _, bar = phi_restate(M[rows], Bs, inc, ua, Pc)
            bars.append(np.stack([2 * (bar[t] + np.abs(ua[:, t, 2:]) @ ub[rows][:, t, 2:].T + ub[rows][:, t, 2:] @ np.abs(ua[:, t, 2:]).T)
                                  for t in range(T)]))
        pa, pb = a["phi"][si], b["phi"][si]
        assert same(np.isnan(pa), np.isnan(pb))
        ok = ~np.isnan(pa)
        # (each bar: the Gram's own, plus what the errors of the run's a_j move Phi by, doubled for the second order)
        assert np.all(np.abs(pa - pb)[ok] <= (bars[0] + bars[1])[ok])
        sa = np.where(a["flipped"][off[si]:off[si] + m] == 1, -1.0, 1.0)
        assert sa.min() == -1.0 and sa.max() == 1.0                           # both codings occur inside the set


def test_a_f32_mfma_handle_gives_the_same_bits():
    N, T, Pc = 257, 2, 3
    G, Y, C, inc, _ = make_set_inputs(N, T, Pc, seed=31)
    sets = make_sets(9)[2:5]
    out = []
    for prec in (_lib.PREC_I8_EXACT, _lib.PREC_F32_MFMA):
        with gpca.GpcaEngine(precision=prec, storage=_lib.STORE_INT8) as e:
            load(e, G)
            out.append(e.assoc_logistic_set(Y, sets, C, include=inc, max_vif=VIF, ua=True))
    a, b = out
    assert all(same(x, y) for x, y in zip(a["phi"], b["phi"])) and same(a["ua"], b["ua"]) and same(a["V"], b["V"])
    assert np.isfinite(a["phi"][1]).any()


def test_error_paths():
    N, T, Pc = 130, 1, 1
    G, Y, C, inc, _ = make_set_inputs(N, T, Pc, seed=3)
    lib = _lib.load()
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        e.upload_genotypes_i8(G)
        with pytest.raises(GpcaError) as ei:                                  # a13's state errors come first
            e.assoc_logistic_set(Y, [[0, 1]], C, include=inc)
        assert ei.value.status == _lib.GPCA_ERR_STATE
        load(e, G)
        good = e.assoc_logistic_set(Y, [[0, 1], [4]], C, include=inc)
        assert good["phi"][0].shape == (1, 2, 2) and good["phi"][1].shape == (1, 1, 1)

        def refused(sets, word, **kw):
            with pytest.raises(GpcaError) as ei:
                e.assoc_logistic_set(Y, sets, C, include=inc, **kw)
            assert ei.value.status == _lib.GPCA_ERR_BAD_ARG and word in str(ei.value), str(ei.value)
        refused([], "n_sets")
        refused([[0, 1], []], "set 1")
        refused([[0], list(range(129))], "set 1")
        refused([[0, 1], [2, 3], [5, 5]], "set 2")
        refused([[0, 1], [7, 3]], "set 1")
        refused([[0, K_ROWS]], "outside")
        refused([[-1, 3]], "outside")
        refused([[0, 1]], "max_vif", max_vif=0.5)
        # a NULL phi, through the C ABI
        vp = lambda a: a.ctypes.data_as(__import__("ctypes").c_void_p)
        Yv, Cv = np.ascontiguousarray(Y), np.ascontiguousarray(C)
        off, rows, st = np.array([0, 2], np.int64), np.array([0, 1], np.int64), np.zeros(10)
        assert lib.gpca_assoc_logistic_set(e._h, vp(Yv), T, vp(Cv), Pc, vp(inc), 50.0, 1, vp(off), vp(rows), vp(st), None, None, None) == _lib.GPCA_ERR_BAD_ARG
        assert b"phi" in lib.gpca_last_error(e._h)
        Ybad = Y.copy()
        Ybad[inc == 1] = 1.0
        with pytest.raises(GpcaError) as ei:                                  # a13's own refusals pass through: one class only
            e.assoc_logistic_set(Ybad, [[0, 1]], C, include=inc)
        assert ei.value.status == _lib.GPCA_ERR_BAD_ARG
        # set_off and set_rows themselves, through the C ABI
        phi = np.zeros(16)

        def raw(n_sets, off_, rows_):
            rc = lib.gpca_assoc_logistic_set(e._h, vp(Yv), T, vp(Cv), Pc, vp(inc), 50.0, n_sets, None if off_ is None else vp(off_),
                                             None if rows_ is None else vp(rows_), None, None, None, vp(phi))
            return rc, lib.gpca_last_error(e._h).decode()
        assert raw(1, off, rows)[0] == _lib.GPCA_OK
        for got, word in ((raw(1, None, rows), "set_off"), (raw(1, off, None), "set_rows"), (raw(0, off, rows), "n_sets"),
                          (raw(-3, off, rows), "n_sets"), (raw(1, np.array([1, 2], np.int64), rows), "set_off[0]")):
            assert got[0] == _lib.GPCA_ERR_BAD_ARG and word in got[1] and "gpca_assoc_logistic_set" in got[1], got
        # K = 0: an empty keep mask
        e.set_standardization(np.ones(K_ROWS, np.float32), np.ones(K_ROWS, np.float32), np.zeros(K_ROWS, np.uint8))
        with pytest.raises(GpcaError) as ei:
            e.assoc_logistic_set(Y, [[0, 1]], C, include=inc)
        assert ei.value.status == _lib.GPCA_ERR_STATE and "no kept row" in str(ei.value)
    # (GPCA_ERR_OOM needs sets whose workspace exceeds the free memory of the card: no shape a quick test can hold reaches it)
    with gpca.GpcaEngine() as e:                                              # a streamed handle
        e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), K_ROWS, N, panel_rows=256, ring_slots=2, fused=False)
        e.snp_stats(gpca.QcConfig.none())
        with pytest.raises(GpcaError) as ei:
            e.assoc_logistic_set(Y, [[0, 1]], C, include=inc)
        assert ei.value.status == _lib.GPCA_ERR_STATE and "panel" in str(ei.value) and "gpca_assoc_logistic_set" in str(ei.value)
    with gpca.GpcaEngine() as e:                                              # a hooked (row-sharded) handle
        e.upload_genotypes_i8(G[:20].copy())
        e.set_allreduce_hook(lambda buf: None, 2, 0, 0)
        e.set_standardization(np.ones(20, np.float32), np.ones(20, np.float32), np.ones(20, np.uint8))
        with pytest.raises(GpcaError) as ei:
            e.assoc_logistic_set(Y, [[0, 1]], C, include=inc)
        assert ei.value.status == _lib.GPCA_ERR_STATE and "shard" in str(ei.value) and "gpca_assoc_logistic_set" in str(ei.value)


# ------------------------------------------------------------------------------------------------ what it is for
def cohort(seed, kind, N=2000, m=20):
    rng = np.random.default_rng(seed)
    maf = np.concatenate([rng.uniform(0.007, 0.01, 5), rng.uniform(0.00025, 0.0005, m - 5)])
    G = np.zeros((m, N), np.int8)
    for j in range(m):                                  # (exact carrier counts: the sample's MAF is the drawn one, rounded down)
        G[j, rng.choice(N, max(int(2 * N * maf[j]), 1), replace=False)] = 1
    eff = np.zeros(m)
    if kind == "mixed":
        eff[:5] = [1.5, -3.0, 1.5, -3.0, 1.5]
    elif kind == "same":
        eff[:5] = 0.8
    eta = eff @ (G - G.mean(1, keepdims=True))
    lo, hi = -10.0, 10.0
    for _ in range(60):
        a = 0.5 * (lo + hi)
        if (1 / (1 + np.exp(-(a + eta)))).mean() > 0.1:
            hi = a
        else:
            lo = a
    Y = (rng.random(N) < 1 / (1 + np.exp(-(a + eta)))).astype(np.float64)
    return G, Y


def beta_weights(a1_freq):
    f = np.minimum(a1_freq, 1.0 - a1_freq)
    return 25.0 * (1.0 - f) ** 24


def cohort_restatement(G, Y):
    _, mu, _ = gpca.GpcaEngine.logistic_null(Y)
    w = mu * (1 - mu)
    Gt = G.astype(np.float64)
    b = Gt @ w
    phi = (Gt * w) @ Gt.T - np.outer(b, b) / w.sum()
    return set_test_reference(Gt @ (Y - mu), phi, beta_weights(Gt.mean(1) / 2))


@pytest.mark.parametrize("store", ["int8", "2bit"])
def test_set_tests_on_a_cohort(store):
    got = {}
    for kind in ("mixed", "same", "null"):
        G, Y = cohort(COHORT_SEED, kind)
        assert 0.08 < Y.mean() < 0.12 and (G.mean(1) / 2).max() <= 0.01
        with gpca.GpcaEngine(storage=STORES[store]) as e:
            load(e, G)
            r = e.assoc_logistic_set(Y, [np.arange(20)], ua=True)
        u = np.where(r["flipped"] == 1, -1.0, 1.0) * r["ua"][:, 0, 0]
        t = gpca.set_test(u, r["phi"][0][0], beta_weights(r["a1_freq"]))
        ref = cohort_restatement(G, Y)
        print(kind, "device: SKAT", t["skat_log10p"], "burden", t["burden_log10p"], " restatement: SKAT", ref["skat_log10p"], "burden",
              ref["burden_log10p"])
        assert t["m_used"] == ref["m_used"] >= 15                           # (a variant without a carrier drops out of both)
        got[kind] = t
    assert got["mixed"]["skat_log10p"] - got["mixed"]["burden_log10p"] >= 2.0
    assert got["same"]["burden_log10p"] - got["same"]["skat_log10p"] >= 0.5
    assert got["null"]["skat_log10p"] < 2.0 and got["null"]["burden_log10p"] < 2.0
