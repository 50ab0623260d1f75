"""gpca_assoc_qtl_cis / gpca_qtl_perm_panel: cis-QTL mapping (assoc_qtl_cis.hip, gpca_assoc_qtl_cis.cpp; gpca.h section a25), through the
C ABI.

Column 0 of a trait's panel is the trans scan restricted to the window, so n_var, best_row, best_r2 and best_stat are held, bit for bit,
to gpca_assoc_qtl over rows = [lo, hi) and to gpca_assoc_linear at the best row (both held to their own models in test_gpu_assoc_qtl.py
and test_gpu_assoc.py).  The permuted columns are held bit for bit where the host step is exact in any order (Pc = 0, integer traits
that sum to 0 over the included samples: gpca_assoc_qtl on the explicitly permuted column then stages the same f32 panel and the same
yy), the panel kernel bit for bit against a numpy loop in the section's order, and the path with covariates within the xb bar of
test_gpu_assoc.py (restate: the f32 rounding of B, the f32 flush groups, the f64 side and the kappa term for the engine's Cholesky basis
against numpy's), as that module derives it and with nothing added, carried to r2: the model multiplies the hook's f32 panel (from
numpy's design) in f64, and d r2 = 2 bar |xb| / (sxx yy) (first order: r2 = xb^2 / (sxx yy), sxx and yy being the engine's own)."""
import ctypes as C
import os

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from genomic_pca_amd._lib import GpcaError
from _edges import edge_keeps
from test_gpu_assoc import design, restate

pytestmark = pytest.mark.gpu

ENGINES = {"int8": dict(storage=_lib.STORE_INT8), "2bit": dict(storage=_lib.STORE_2BIT),
           "f32": dict(storage=_lib.STORE_INT8, precision=_lib.PREC_F32_MFMA)}
VIF = 50.0
MISSING = -127
DEAD0, DEAD1 = 200, 204                   # kept rows [200, 204) are monomorphic over the included samples


@pytest.fixture
def tw_env():
    old = os.environ.get("GPCA_QTL_TW")

    def set_tw(tw):
        if tw is None:
            os.environ.pop("GPCA_QTL_TW", None)
        else:
            os.environ["GPCA_QTL_TW"] = str(tw)
    yield set_tw
    if old is None:
        os.environ.pop("GPCA_QTL_TW", None)
    else:
        os.environ["GPCA_QTL_TW"] = old


def make_inputs(M, N, G, Pc, seed, miss=0.02, keep=None):
    """calls with about 2 % missing, an include mask that excludes sample 1 and about one sample in ten (their calls are missing, their
    traits and covariates extreme), traits and covariates.  Among the kept rows, [DEAD0, DEAD1) are monomorphic over the included
    samples and row 9 has no observed call."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, M)[:, None]
    Gm = ((rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)).astype(np.int8)
    inc = np.ones(N, np.uint8)
    inc[1] = 0
    if N >= 40:
        inc[rng.random(N) < 0.1] = 0
    Gm[rng.random((M, N)) < miss] = MISSING
    kept = np.arange(M) if keep is None else np.flatnonzero(keep)
    if kept.size > DEAD1:
        Gm[kept[DEAD0:DEAD1]] = 2
        Gm[kept[9]] = MISSING
    Gm[:, inc == 0] = MISSING
    Y = rng.standard_normal((N, G))
    Cv = rng.standard_normal((N, Pc))
    Y[inc == 0] = 1e30
    Cv[inc == 0] = -1e30
    return Gm, Y, Cv, inc


def load(e, Gm, keep=None):
    e.upload_genotypes_i8(Gm)
    M = Gm.shape[0]
    e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.ones(M, np.uint8) if keep is None else keep)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def windows_for(K):
    w = [(5, 5), (7, 8), (127, 129), (37, 250), (0, K), (DEAD0, DEAD1), (130, 131), (128, 256), (K - 1, K), (K, K)]
    return [(lo, hi) for lo, hi in w if 0 <= lo <= hi <= K] + [(0, 0)]


# ------------------------------------------------------------------------------------------------ 1. column 0 = the trans scan on the window
CASES1 = [(N, name) for N in (17, 64, 65, 257) for name in ("every row", "last block dropped", "one row")]


@pytest.mark.parametrize("N,keep_name", CASES1, ids=[f"N{n}-{k.replace(' ', '_')}" for n, k in CASES1])
def test_column_0_is_the_trans_scan_on_the_window(N, keep_name):
    M = 300 if keep_name == "every row" else 330
    keep = dict(edge_keeps(M))[keep_name]
    K = int(keep.sum())
    win = np.array(windows_for(K), np.int64)
    G = len(win)
    Pc = 2
    Gm, Y, Cv, inc = make_inputs(M, N, G, Pc, seed=100 + N, keep=keep)
    n = int(inc.sum())
    eng = ("int8", "2bit", "f32")[(N + K) % 3]
    P = 3 if N % 2 else 0
    with gpca.GpcaEngine(**ENGINES[eng]) as e:
        load(e, Gm, keep)
        q = e.assoc_qtl_cis(Y, win, Cv, include=inc, max_vif=VIF, n_perm=P, seed=4)
        assert q["perm_r2"].shape == (G, P) and q["df"] == n - Pc - 2
        n_live = 0
        for g, (lo, hi) in enumerate(win.tolist()):
            t = e.assoc_qtl(Y[:, g:g + 1], Cv, include=inc, max_vif=VIF, r2_min=1.0, rows=(lo, hi))
            with np.errstate(all="ignore"):
                live = ~((t["n_obs"] == 0) | ~(t["xx"] > 0.0) | (t["sxx"] * VIF < t["xx"]))
            assert q["n_var"][g] == int(live.sum()), (g, lo, hi)
            assert q["best_row"][g] == t["best_row"][0] and same(q["best_r2"][g], t["best_r2"][0]), (g, lo, hi)
            if live.any():
                n_live += 1
                br = int(q["best_row"][g])
                assert lo <= br < hi
                a = e.assoc_linear(Y[:, g:g + 1], Cv, include=inc, max_vif=VIF, rows=(br, br + 1), xb=True)
                assert q["best_stat"][g, 0] == a["xb"][0, 0] and q["best_stat"][g, 1] == a["sxx"][0] and q["best_stat"][g, 2] == t["yy"][0]
                assert not np.isnan(q["perm_r2"][g]).any()
            else:
                assert q["best_row"][g] == -1 and np.isnan(q["best_r2"][g]) and np.isnan(q["best_stat"][g]).all()
                assert np.isnan(q["perm_r2"][g]).all()
        assert n_live >= (5 if K > DEAD1 else 1)
        if K > DEAD1:
            assert q["n_var"][windows_for(K).index((DEAD0, DEAD1))] == 0


# ------------------------------------------------------------------------------------------------ 2. the permutation path, bit for bit
def integer_traits(rng, N, G, inc):
    """integer-valued traits that sum to exactly 0 over the included samples: centring, the f32 rounding and yy are exact in any order"""
    s = np.flatnonzero(inc)
    Y = rng.integers(-6, 7, (N, G)).astype(np.float64)
    Y[s[-1]] -= Y[s].sum(0)
    assert (Y[s].sum(0) == 0).all() and (np.abs(Y[s]) < 2 ** 11).all() and (Y[s].std(0) > 0).all()
    Y[inc == 0] = 1e30
    return Y


@pytest.mark.parametrize("tw", [None, 64])
@pytest.mark.parametrize("P", [1, 62, 63, 64, 127])
def test_permuted_columns_equal_the_trans_scan_on_permuted_traits(P, tw, tw_env):
    M, N = 300, 130
    Gm, _, _, inc = make_inputs(M, N, 1, 0, seed=300 + P)
    rng = np.random.default_rng(P)
    win = np.array([(37, 250), (127, 129), (0, M)], np.int64)
    Y = integer_traits(rng, N, len(win), inc)
    s = np.flatnonzero(inc)
    perm = gpca.qtl_perm_table(11, s.size, P)
    tw_env(tw)
    with gpca.GpcaEngine(**ENGINES["2bit" if P % 2 else "int8"]) as e:
        load(e, Gm)
        q = e.assoc_qtl_cis(Y, win, None, include=inc, max_vif=VIF, perm=perm)
        for g, (lo, hi) in enumerate(win.tolist()):
            Yp = np.full((N, P), 1e30)
            Yp[s] = Y[s, g][perm].T                                   # column p: sample S[i] holds y[S[perm[p][i]]]
            t = e.assoc_qtl(Yp, None, include=inc, max_vif=VIF, r2_min=1.0, rows=(lo, hi))
            assert np.array_equal(q["perm_r2"][g], t["best_r2"]), (g, P, tw)
            assert (t["yy"] == q["best_stat"][g, 2]).all()
            t0 = e.assoc_qtl(Y[:, g:g + 1], None, include=inc, max_vif=VIF, r2_min=1.0, rows=(lo, hi))
            assert q["best_r2"][g] == t0["best_r2"][0] and q["best_row"][g] == t0["best_row"][0]


# ------------------------------------------------------------------------------------------------ 3. the panel kernel
def panel_np(b, Q, perm):
    """a25's step 3 in numpy f64, one rounding per operation (numpy fuses nothing): [P][n] float32"""
    P, n = perm.shape
    v = b[perm]                                                        # [P][n]
    Pc = Q.shape[1]
    if Pc == 0:
        return v.astype(np.float32)
    c = np.zeros((P, Pc))
    for i in range(n):                                                 # c_j = sum_i Q_ij v_i, i ascending
        c = c + Q[i][None, :] * v[:, i][:, None]
    sacc = np.zeros((P, n))
    for j in range(Pc):                                                # s_i = sum_j Q_ij c_j, j ascending
        sacc = sacc + Q[:, j][None, :] * c[:, j][:, None]
    return (v - sacc).astype(np.float32)


@pytest.fixture(scope="module")
def engine():
    with gpca.GpcaEngine() as e:
        yield e


@pytest.mark.parametrize("n", [3, 64, 65, 1000])
@pytest.mark.parametrize("Pc", [0, 1, 7, 63])
def test_panel_kernel_equals_the_numpy_loop(engine, Pc, n):
    rng = np.random.default_rng(1000 * Pc + n)
    b = rng.standard_normal(n)
    Q = rng.standard_normal((n, Pc)) / np.sqrt(n)
    for P in (1, 65):
        perm = gpca.qtl_perm_table(5, n, P)
        perm[0] = np.arange(n)                                          # the identity
        if P > 1:
            perm[1] = np.arange(n)[::-1]                                # a reversal
        got = engine.qtl_perm_panel(b, Q, perm)
        assert got.dtype == np.float32 and got.shape == (P, n)
        assert np.array_equal(got, panel_np(b, Q, perm)), (Pc, n, P)
    if Pc == 0:
        assert np.array_equal(got[1], b[::-1].astype(np.float32))


def test_panel_kernel_gathers_from_global_memory_past_the_lds_limit(engine):
    n = 4097                                                            # kQtlPermLdsSamples + 1 (plan_math.h)
    rng = np.random.default_rng(8)
    b, Q = rng.standard_normal(n), rng.standard_normal((n, 2)) / 64.0
    perm = gpca.qtl_perm_table(6, n, 3)
    assert np.array_equal(engine.qtl_perm_panel(b, Q, perm), panel_np(b, Q, perm))
    n = 4096
    perm = gpca.qtl_perm_table(6, n, 2)
    assert np.array_equal(engine.qtl_perm_panel(b[:n], Q[:n], perm), panel_np(b[:n], Q[:n], perm))


# ------------------------------------------------------------------------------------------------ 4. with covariates, within the xb bar
SEED4 = 4000                  # a seed where the model's best and runner-up r2 of every column are more than twice the bar apart (asserted)


def test_permuted_columns_with_covariates_within_the_bar():
    M, N, Pc, P = 300, 257, 5, 65
    win = np.array([(37, 250), (0, 300)], np.int64)
    Gm, Y, Cv, inc = make_inputs(M, N, len(win), Pc, seed=SEED4)
    s = np.flatnonzero(inc)
    perm = gpca.qtl_perm_table(SEED4, s.size, P)
    B, _, _, kappa = design(Y, Cv, inc)
    Q = B[s][:, len(win):]
    with gpca.GpcaEngine() as e:
        load(e, Gm)
        q = e.assoc_qtl_cis(Y, win, Cv, include=inc, max_vif=VIF, perm=perm)
        info = e.assoc_qtl(Y, Cv, include=inc, max_vif=VIF, r2_min=1.0)
        panels = [e.qtl_perm_panel(B[s, g], Q, perm) for g in range(len(win))]
    with np.errstate(all="ignore"):
        live = ~((info["n_obs"] == 0) | ~(info["xx"] > 0.0) | (info["sxx"] * VIF < info["xx"]))
    worst = 0.0
    for g, (lo, hi) in enumerate(win.tolist()):
        Bp = np.zeros((N, P))
        Bp[s] = panels[g].T.astype(np.float64)
        ref = restate(Gm[lo:hi], Bp, inc, kappa, Pc)
        bar = ref["bar"]
        lv = live[lo:hi]
        den = (info["sxx"][lo:hi, None] * info["yy"][g])[lv]
        xb, bar = ref["xb"][lv], bar[lv]
        r2 = xb * xb / den
        bar2 = 2.0 * bar * np.abs(xb) / den
        top = np.argsort(r2, axis=0)[::-1][:2]                          # best and runner-up row of every column
        cols = np.arange(P)
        gap = r2[top[0], cols] - r2[top[1], cols]
        both = bar2[top[0], cols] + bar2[top[1], cols]
        assert (gap > 2.0 * np.maximum(bar2[top[0], cols], bar2[top[1], cols])).all() and (gap > both).all(), "pick another SEED4"
        err = np.abs(q["perm_r2"][g] - r2[top[0], cols])
        worst = max(worst, float(np.max(err / bar2[top[0], cols])))
        assert (err <= bar2[top[0], cols]).all()
    print("perm_r2: max err / bar", worst, "kappa", kappa)


# ------------------------------------------------------------------------------------------------ 5. invariance
def test_invariance_to_order_split_storage_and_repetition(tw_env):
    M, N, Pc, P = 300, 130, 3, 70
    win = np.array([(37, 250), (127, 129), (0, 300), (5, 5), (DEAD0, DEAD1), (100, 101)], np.int64)
    G = len(win)
    Gm, Y, Cv, inc = make_inputs(M, N, G, Pc, seed=55)
    perm = gpca.qtl_perm_table(2, int(inc.sum()), P)
    keys = ("n_var", "best_row", "best_r2", "best_stat", "perm_r2")
    out = {}
    for name, kw in ENGINES.items():
        with gpca.GpcaEngine(**kw) as e:
            load(e, Gm)
            out[name] = e.assoc_qtl_cis(Y, win, Cv, include=inc, max_vif=VIF, perm=perm)
            if name == "int8":
                again = e.assoc_qtl_cis(Y, win, Cv, include=inc, max_vif=VIF, perm=perm)
                rev = e.assoc_qtl_cis(Y[:, ::-1], win[::-1], Cv, include=inc, max_vif=VIF, perm=perm)
                a = e.assoc_qtl_cis(Y[:, :2], win[:2], Cv, include=inc, max_vif=VIF, perm=perm)
                b = e.assoc_qtl_cis(Y[:, 2:], win[2:], Cv, include=inc, max_vif=VIF, perm=perm)
                tw_env(64)
                narrow = e.assoc_qtl_cis(Y, win, Cv, include=inc, max_vif=VIF, perm=perm)
                tw_env(None)
    ref = out["int8"]
    assert (ref["n_var"] > 0).sum() == 4 and not np.isnan(ref["perm_r2"][ref["n_var"] > 0]).any()
    for k in keys:
        assert same(ref[k], again[k]), k
        assert same(ref[k], rev[k][::-1]), k
        assert same(ref[k], np.concatenate([a[k], b[k]])), k
        assert same(ref[k], narrow[k]), k
        assert same(ref[k], out["2bit"][k]) and same(ref[k], out["f32"][k]), k


# ------------------------------------------------------------------------------------------------ 6. planted signal
SEED6 = 606


def test_planted_signal_and_a_null_trait():
    M, N, Pc, P = 400, 400, 2, 500
    lo, hi = 100, 300
    Gm, Y, Cv, inc = make_inputs(M, N, 2, Pc, seed=SEED6)
    rng = np.random.default_rng(SEED6)
    s = inc == 1
    snp = lo + 5 + int(np.argmax(np.where(Gm == MISSING, 0, Gm).astype(np.float64).var(1)[lo + 5:hi]))
    g = np.where(Gm[snp] == MISSING, 0, Gm[snp]).astype(np.float64)
    Y[s, 0] = 0.8 * g[s] + rng.standard_normal(int(s.sum()))           # trait 0 follows the SNP; trait 1 is noise
    win = np.array([(lo, hi), (lo, hi)], np.int64)
    with gpca.GpcaEngine() as e:
        load(e, Gm)
        q = e.assoc_qtl_cis(Y, win, Cv, include=inc, max_vif=VIF, n_perm=P, seed=SEED6)
    assert q["best_row"][0] == snp and (q["n_var"] > 190).all()
    hit = gpca.qtl_beta_approx(q["perm_r2"][0], q["best_r2"][0], q["df"])
    null = gpca.qtl_beta_approx(q["perm_r2"][1], q["best_r2"][1], q["df"])
    print("planted:", hit, "null:", null)
    assert hit["pval_perm"] == 1.0 / 501.0 and hit["log10p_beta"] > 6.0
    assert 0.05 < null["pval_perm"] < 0.95 and null["status"] == 0
    assert abs(null["log10p_beta"] + np.log10(null["pval_perm"])) < 0.3
    t = gpca.qtl_stats(*q["best_stat"][0], q["df"])[0, 2]
    assert abs(t) > 8.0


# ------------------------------------------------------------------------------------------------ 7. errors
def test_errors():
    rng = np.random.default_rng(2)
    M, N = 40, 50
    Gm = rng.integers(0, 3, (M, N)).astype(np.int8)
    Y, Cv = rng.standard_normal((N, 3)), rng.standard_normal((N, 2))
    win = np.array([(0, 10), (5, 40), (7, 7)], np.int64)
    perm = gpca.qtl_perm_table(0, N, 4)
    BA, ST = _lib.GPCA_ERR_BAD_ARG, _lib.GPCA_ERR_STATE

    def err(e, Y=Y, win=win, Cv=Cv, **kw):
        kw.setdefault("perm", perm)
        with pytest.raises(GpcaError) as ei:
            e.assoc_qtl_cis(Y, win, Cv, **kw)
        return ei.value.status, str(ei.value)

    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(Gm)
        assert err(e)[0] == ST                                                            # no standardisation
        load(e, Gm, np.zeros(M, np.uint8))
        assert err(e)[0] == ST                                                            # K = 0
        load(e, Gm)
        assert e.assoc_qtl_cis(Y, win, Cv, perm=perm)["perm_r2"].shape == (3, 4)
        for bad in ((-1, 5), (6, 5), (0, M + 1)):
            w = win.copy(); w[1] = bad
            st, msg = err(e, win=w)
            assert st == BA and "trait 1" in msg, bad
        assert err(e, Cv=rng.standard_normal((N, 64)))[0] == BA                           # Pc > 63
        assert err(e, max_vif=0.5)[0] == BA
        Yb = Y.copy(); Yb[7, 2] = np.inf
        assert "Y[7][2]" in err(e, Y=Yb)[1]
        Yc = Y.copy(); Yc[:, 1] = 3.0
        assert "trait 1" in err(e, Y=Yc)[1]
        # a table row that is not a permutation: a repeated index, an index out of range
        pb = perm.copy(); pb[2, 5] = pb[2, 6]
        st, msg = err(e, perm=pb)
        assert st == BA and "row 2" in msg
        pb = perm.copy(); pb[3, 0] = N
        st, msg = err(e, perm=pb)
        assert st == BA and "row 3" in msg
        inc = np.ones(N, np.uint8); inc[4] = 0
        with pytest.raises(ValueError):
            e.assoc_qtl_cis(Y, win, Cv, include=inc, perm=perm)                          # the table is over the 49 included samples
        st, msg = err(e, include=inc, perm=np.where(perm[:, :N - 1] >= N - 1, 0, perm[:, :N - 1]))
        assert st == BA and "not a permutation" in msg
        st, msg = (lambda ei: (ei.value.status, str(ei.value)))(pytest.raises(GpcaError, e.qtl_perm_panel, Y[:, 0], Cv, pb))
        assert st == BA and "row 3" in msg
        # P and the pointer rules, through the C ABI itself
        lib = _lib.load()
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        Yv, Cvv = np.ascontiguousarray(Y), np.ascontiguousarray(Cv)
        nv, bw, b2, bs, pr = np.zeros(3, np.int64), np.zeros(3, np.int64), np.zeros(3), np.zeros((3, 3)), np.zeros((3, 4))
        call = lambda permp, P, prp=pr, winp=win, nvp=nv: lib.gpca_assoc_qtl_cis(e._h, vp(Yv), 3, vp(Cvv), 2, None, 50.0, vp(winp), vp(permp), P,
                                                                                 vp(nvp), vp(bw), vp(b2), vp(bs), vp(prp))
        assert call(perm, 4) == _lib.GPCA_OK
        assert call(None, 4) == BA and call(perm, -1) == BA and call(perm, 65536) == BA and call(perm, 4, prp=None) == BA
        assert call(None, 0, prp=None) == _lib.GPCA_OK
        assert call(perm, 4, winp=None) == BA and call(perm, 4, nvp=None) == BA
        Gb = Gm.copy(); Gb[17, 9] = 3
        load(e, Gb)
        st, msg = err(e)
        assert st == _lib.GPCA_ERR_INVALID_GENOTYPE and "row 17" in msg
        assert e.assoc_qtl_cis(Y, np.array([(0, 10), (3, 17), (7, 7)]), Cv, perm=perm)["n_var"][0] > 0   # windows that do not read the row
    with gpca.GpcaEngine() as e:                                                         # a streamed handle
        e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: Gm[r0:r0 + r]), M, N, panel_rows=256, ring_slots=2, fused=False)
        e.snp_stats(gpca.QcConfig.none())
        st, msg = err(e)
        assert st == ST and "panel" in msg
    with gpca.GpcaEngine() as e:                                                         # a hooked (row-sharded) handle
        e.upload_genotypes_i8(Gm[:20].copy())
        e.set_allreduce_hook(lambda buf: None, 2, 0, 0)
        e.set_standardization(np.ones(20, np.float32), np.ones(20, np.float32), np.ones(20, np.uint8))
        st, msg = err(e, win=np.array([(0, 10), (5, 20), (7, 7)]))
        assert st == ST and "shard" in msg
