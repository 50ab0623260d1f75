"""gpca_admix_step_holdout and gpca_admix_cv (admix.hip, gpca_admix.cpp; include/gpca.h section a22) through the C ABI.

The hold-out step is held to the plain step, bit for bit: its Q', F' and loglik on G must be those of gpca_admix_step on G with the fold's
calls overwritten by the missing code (the fold from the numpy philox restatement in _admix_cv.py).  The held-out counts are exact; the
held-out log-likelihood is held to tests/test_gpu_admix.py's derived bar ll_bar(K, n, ref) = 2 (2 K + 4) u 2 n + C_LOG u |ref| (restated in
_admix_cv.py, C_LOG = 3 as measured there).  gpca_admix_cv is held, with ==, to the chain it documents: gpca_admix on the masked matrix,
then one hold-out step on the whole matrix at the returned parameters.

The choice of K (test_cv_error_chooses_k): 600 SNPs x 96 samples, K = 3, Balding-Nichols Fst 0.1, Q ~ Dirichlet(0.3) with 10 pure samples
per ancestry, 2 % missing; v = 5, cv_seed 0, tol 1e-6, seed 7.  The f64 numpy model with the philox folds from a21's init gives
cv_error 1.188162 / 1.161170 / 1.150608 / 1.219920 for K = 1 .. 4: gaps cv(2) - cv(3) = 0.010562 and cv(4) - cv(3) = 0.069312, against a
per-fold scatter of about 0.015 that is common to every K (K = 3, per fold: 1.1348, 1.1599, 1.1563, 1.1687, 1.1335).
Measured on an MI355X: cv_error 1.188162 / 1.160873 / 1.150350 / 1.226779; steps per fold 7 at K = 1, 109 .. 178 at K = 2, 175 .. 235 at
K = 3, 226 .. 364 at K = 4.  |cv_device - cv_model| = 2.970e-4 at K = 2 and 2.579e-4 at K = 3: not derivable, since the two stop at
different steps (the device's stopping rule sees f32-evaluated log-likelihoods, as tests/test_gpu_admix.py records).  The test holds
both to twice the larger figure, 5.94e-4, which must -- and does -- stay below a fifth of the model's cv(2) - cv(3), 2.11e-3."""
import ctypes

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from genomic_pca_amd._lib import GpcaError

import _admix_cv as A
from _admix_cv import EPS, MISSING, folds_np, hold, ll_bar
from _edges import edge_keeps

pytestmark = pytest.mark.gpu

STORES = {"int8": _lib.STORE_INT8, "2bit": _lib.STORE_2BIT}
ROWBLOCK = 4096


def make(M, N, seed, miss=0.02):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.95, M)[:, None]
    G = (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)
    G[rng.random((M, N)) < miss] = MISSING
    return G


def theta(Kr, N, K, seed):
    rng = np.random.default_rng(seed)
    Q = rng.dirichlet(np.full(K, 0.5), N).astype(np.float32)
    Q = np.maximum(Q, EPS)
    Q = (Q / Q.sum(1, keepdims=True, dtype=np.float32)).astype(np.float32)
    return Q, rng.uniform(0.02, 0.98, (Kr, K)).astype(np.float32)


def load(e, G, keep=None):
    e.upload_genotypes_i8(G)
    M = G.shape[0]
    e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.ones(M, np.uint8) if keep is None else keep)


def masked(G, keep, fold, c):
    """G with the observed calls of fold c among the kept rows overwritten by the missing code (the fold is indexed by kept row)"""
    out = G.copy()
    rows = np.flatnonzero(keep) if keep is not None else np.arange(G.shape[0])
    out[rows] = hold(G[rows], fold, c)
    return out


def check_mask(ea, eb, G, K, v, cs, seed, keep=None, mode=None, what=None):
    """the hold-out step (v, c) of ea (which holds G) against the plain step of eb on the masked matrix; returns the hold-out results"""
    Kr = G.shape[0] if keep is None else int(keep.sum())
    N = G.shape[1]
    Q, F = theta(Kr, N, K, seed=seed)
    fold = folds_np(seed, v, Kr, N)
    assert np.array_equal(fold, gpca.admix_cv_fold(seed, v, Kr, N)) and fold.max(initial=0) < v, what
    out = {}
    for c in cs:
        r = ea.admix_step_holdout(Q, F, v, c, cv_seed=seed, mode=mode)
        load(eb, masked(G, keep, fold, c), keep)
        Qn, Fn, ll = eb.admix_step(Q, F, mode)
        assert np.array_equal(r["Q"], Qn) and np.array_equal(r["F"], Fn) and r["loglik"] == ll, (what, v, c)
        Gk = G if keep is None else G[keep != 0]
        m = (fold == c) & (Gk != MISSING)
        assert r["n_held"] == int(m.sum()) and r["n_het_held"] == int((Gk[m] == 1).sum()), (what, v, c)
        out[c] = (r, Q, F, m)
    return out


# ---- 1. the mask is exact ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("store", sorted(STORES))
def test_rows_at_quad_tile_and_block_edges(store):
    """kept rows at the edges of a quad of 4, a tile of 16 and a block of 4 096: the quad index is global, not local to a tile or block"""
    with gpca.GpcaEngine(storage=STORES[store]) as ea, gpca.GpcaEngine(storage=STORES[store]) as eb:
        for M in (1, 3, 4, 5, 16, 17, ROWBLOCK - 1, ROWBLOCK + 1, 2 * ROWBLOCK + 1):
            G = make(M, 17, seed=M)
            load(ea, G)
            check_mask(ea, eb, G, 3, 5, range(5) if M <= 17 else (1, 4), seed=1000 + M, what=("rows", M))


@pytest.mark.parametrize("store", sorted(STORES))
def test_samples_at_group_and_chunk_edges(store):
    with gpca.GpcaEngine(storage=STORES[store]) as ea, gpca.GpcaEngine(storage=STORES[store]) as eb:
        for N in (1, 17, 255, 256, 257, 513):
            G = make(21, N, seed=50 + N)
            load(ea, G)
            check_mask(ea, eb, G, 3, 2, range(2), seed=(1 << 63) - 1 - N, what=("N", N))


@pytest.mark.parametrize("store", sorted(STORES))
def test_every_register_width_and_modes(store):
    """K = 1, 3 (4 registers), 8 (8), 9, 16 (16); a mode vector with references and projected samples; v = 64"""
    M, N = 70, 130
    G = make(M, N, seed=3)
    mode = np.zeros(N, np.uint8); mode[[0, 5, 129]] = 1; mode[[1, 6, 64]] = 2
    with gpca.GpcaEngine(storage=STORES[store]) as ea, gpca.GpcaEngine(storage=STORES[store]) as eb:
        load(ea, G)
        for K in (1, 3, 8, 9, 16):
            got = check_mask(ea, eb, G, K, 64, (0, 63), seed=300 + K, mode=mode, what=("K", K))
            r, Q, _, _ = got[63]
            assert np.array_equal(r["Q"][mode == 1], Q[mode == 1])
        check_mask(ea, eb, G, 3, 5, range(5), seed=77, mode=None, what="no mode")


@pytest.mark.parametrize("store", sorted(STORES))
def test_keep_masks_index_the_fold_by_kept_row(store):
    """the fold's row index is the position among the kept rows, not the original row"""
    M, N = 70, 40
    G = make(M, N, seed=4)
    every_other = np.zeros(M, np.uint8); every_other[1::2] = 1
    ragged = np.ones(M, np.uint8); ragged[[0, 1, 2, 9, 33]] = 0
    mode = np.zeros(N, np.uint8); mode[3] = 1; mode[4] = 2
    with gpca.GpcaEngine(storage=STORES[store]) as ea, gpca.GpcaEngine(storage=STORES[store]) as eb:
        for what, keep in edge_keeps(M) + [("every other row", every_other), ("ragged", ragged)]:
            load(ea, G, keep)
            check_mask(ea, eb, G, 3, 5, range(5), seed=400, keep=keep, mode=mode, what=what)


@pytest.mark.parametrize("store", sorted(STORES))
def test_a_sample_whose_only_call_is_held_keeps_its_row(store):
    """one kept row, v = 2: a sample whose only call is held has no observed call left and keeps its Q row; with every contributor's
    call held (N = 1) the F row stays too"""
    with gpca.GpcaEngine(storage=STORES[store]) as ea, gpca.GpcaEngine(storage=STORES[store]) as eb:
        for N in (1, 17):
            G = make(1, N, seed=5 + N, miss=0.0)
            load(ea, G)
            got = check_mask(ea, eb, G, 3, 2, range(2), seed=500 + N, what=("one row", N))
            seen = 0
            for c, (r, Q, F, m) in got.items():
                held = m[0]
                assert np.array_equal(r["Q"][held], Q[held]) and (not (~held).any() or not np.array_equal(r["Q"][~held], Q[~held]))
                if held.all():
                    assert np.array_equal(r["F"], F) and r["loglik"] == 0.0
                seen += int(held.sum())
            assert seen == N


# ---- 2. the held-out sums ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(70, 300, 3, 5), (ROWBLOCK + 5, 40, 9, 2), (33, 257, 16, 64)])
def test_held_out_sums(shape):
    M, N, K, v = shape
    G = make(M, N, seed=21)
    Q, F = theta(M, N, K, seed=2100)
    fold = folds_np(9, v, M, N)
    n_obs = int((G != MISSING).sum())
    with gpca.GpcaEngine(storage=_lib.STORE_2BIT) as e:
        load(e, G)
        _, _, ll = e.admix_step(Q, F)
        tot_n = 0
        tot_hl = 0.0
        for c in range(v):
            r = e.admix_step_holdout(Q, F, v, c, cv_seed=9)
            m = (fold == c) & (G != MISSING)
            assert r["n_held"] == int(m.sum()) and r["n_het_held"] == int((G[m] == 1).sum()), c
            want = A.loglik64(G, Q, F, m)
            print(f"fold {c}: held_loglik {r['held_loglik']!r} f64 {want!r} bar {ll_bar(K, r['n_held'], want):.3e}")
            assert abs(r["held_loglik"] - want) <= ll_bar(K, r["n_held"], want), c
            assert abs(r["loglik"] + r["held_loglik"] - ll) <= ll_bar(K, n_obs, ll), c    # train + held = the plain step's loglik
            tot_n += r["n_held"]; tot_hl += r["held_loglik"]
        assert tot_n == n_obs
        assert abs(tot_hl - ll) <= ll_bar(K, n_obs, ll)


# ---- 3. bits ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(70, 300, 3), (ROWBLOCK + 5, 40, 9)])
def test_storages_and_precisions_give_the_same_bits(shape):
    M, N, K = shape
    G = make(M, N, seed=11)
    Q, F = theta(M, N, K, seed=1100)
    mode = np.zeros(N, np.uint8); mode[3] = 1; mode[4] = 2
    keys = ("Q", "F", "loglik", "held_loglik", "n_held", "n_het_held")
    got = []
    for store, prec in ((_lib.STORE_INT8, _lib.PREC_DEFAULT), (_lib.STORE_2BIT, _lib.PREC_DEFAULT), (_lib.STORE_INT8, _lib.PREC_F32_MFMA)):
        with gpca.GpcaEngine(precision=prec, storage=store) as e:
            load(e, G)
            got.append(e.admix_step_holdout(Q, F, 5, 2, cv_seed=3, mode=mode))
            again = e.admix_step_holdout(Q, F, 5, 2, cv_seed=3, mode=mode)               # two calls in a row
            assert all(np.array_equal(got[-1][k], again[k]) for k in keys)
    for g in got[1:]:
        assert all(np.array_equal(g[k], got[0][k]) for k in keys)
    assert got[0]["n_held"] > 0 and got[0]["held_loglik"] < 0.0


# ---- 4. the CV is the chain it claims to be ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("accel", [True, False])
@pytest.mark.parametrize("max_iter", [5, 400])
def test_cv_is_the_fit_on_the_masked_matrix_then_one_hold_out_step(accel, max_iter):
    M, N, K, v, cvs = 200, 60, 3, 3, 12
    G = make(M, N, seed=31)
    fold = folds_np(cvs, v, M, N)
    mode = np.zeros(N, np.uint8); mode[2] = 2; mode[5] = 1
    kw = dict(seed=4, max_iter=max_iter, tol=1e-7, accel=accel, mode=mode)
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as ea, gpca.GpcaEngine(storage=_lib.STORE_INT8) as eb:
        load(ea, G)
        Q0, F0 = ea.admix_init(K, seed=4)
        cv = ea.admix_cv(K, folds=v, cv_seed=cvs, **kw)
        cv1 = ea.admix_cv(K, folds=v, cv_seed=cvs, Q=Q0, F=F0, **kw)                       # the same start, handed in
        assert cv1 == cv
        dev, held = 0.0, 0
        for c in range(v):
            load(eb, hold(G, fold, c))
            r = eb.admix(K, Q=Q0, F=F0, **kw)                                             # (the init of G, not of the masked matrix)
            s = ea.admix_step_holdout(r["Q"], r["F"], v, c, cv_seed=cvs, mode=mode)
            f = cv["folds"][c]
            assert (f["steps"], f["cycles"], f["converged"], f["fallbacks"]) == (r["steps"], r["cycles"], r["converged"], r["fallbacks"]), c
            assert f["loglik"] == r["loglik"] and f["held_loglik"] == s["held_loglik"], c
            assert f["n_held"] == s["n_held"] and f["n_het_held"] == s["n_het_held"], c
            assert f["deviance"] == -2.0 * s["held_loglik"] - 4.0 * np.log(2.0) * s["n_het_held"], c
            dev += f["deviance"]; held += f["n_held"]
        assert cv["cv_error"] == dev / held and held == int((G != MISSING).sum())
        if max_iter == 5:
            assert all(f["steps"] == 5 and not f["converged"] for f in cv["folds"])


# ---- 5. it chooses K --------------------------------------------------------------------------------------------------------------------

CV_GAP_MEASURED = 2.970e-4  # max over K = 2, 3 of |cv_device - cv_model| as measured on an MI355X (module docstring)


def test_cv_error_chooses_k():
    G = A.simulate()
    M, N = G.shape
    v, tol = 5, 1e-6
    fold = folds_np(0, v, M, N)
    cv, model = {}, {}
    with gpca.GpcaEngine(storage=_lib.STORE_2BIT) as e:
        load(e, G)
        for K in (1, 2, 3, 4):
            cv[K] = e.admix_cv(K, folds=v, cv_seed=0, seed=7, tol=tol)
            assert all(f["converged"] for f in cv[K]["folds"]), K
        for K in (2, 3):
            model[K] = A.model_cv(G, *e.admix_init(K, seed=7), fold, v, tol)[0]
    for K in sorted(cv):
        print(f"K = {K}: cv_error {cv[K]['cv_error']!r}" + (f" model {model[K]!r} |diff| {abs(cv[K]['cv_error'] - model[K]):.3e}" if K in model else "")
              + f" steps {[f['steps'] for f in cv[K]['folds']]}")
    c = {K: cv[K]["cv_error"] for K in cv}
    assert c[3] < c[2] < c[1] and c[3] < c[4]
    assert model[3] < model[2]
    bar = 2.0 * CV_GAP_MEASURED
    assert bar < (model[2] - model[3]) / 5.0                                             # the bar separates the Ks it is meant to tell apart
    for K in (2, 3):
        assert abs(c[K] - model[K]) <= bar, K


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------------

def test_error_paths():
    M, N, K = 40, 130, 3
    G = make(M, N, seed=14)
    Q, F = theta(M, N, K, seed=1400)
    lib = _lib.load()
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    calls = ("gpca_admix_step_holdout", "gpca_admix_cv")

    def each(e, status, word):
        for name, fn in zip(calls, (lambda: e.admix_step_holdout(Q, F, 5, 0), lambda: e.admix_cv(K, max_iter=1))):
            with pytest.raises(GpcaError) as ei:
                fn()
            assert ei.value.status == status and word in str(ei.value) and name + ":" in str(ei.value), (name, str(ei.value))

    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        e.upload_genotypes_i8(G)
        each(e, _lib.GPCA_ERR_STATE, "standardisation")
        load(e, G)
        Qn, Fn = np.zeros_like(Q), np.zeros_like(F)
        d = [ctypes.c_double(), ctypes.c_double()]
        n = [ctypes.c_int64(), ctypes.c_int64()]

        def step(folds=5, fold=0, q=Q, qn=Qn, ll=d[0], hl=d[1], nh=n[0], nhet=n[1], k=K):
            ref = lambda x: None if x is None else ctypes.byref(x)
            rc = lib.gpca_admix_step_holdout(e._h, k, vp(q), vp(F), None, folds, fold, 0, vp(qn), vp(Fn), ref(ll), ref(hl), ref(nh), ref(nhet))
            return rc, lib.gpca_last_error(e._h).decode()

        def cvf(par=(K, 1, 0, 1e-7, 1, 0), folds=5, q=None, f=None, out=True, err=True):
            o = (_lib.gpca_admix_cv_fold_info * 64)()
            rc = lib.gpca_admix_cv(e._h, ctypes.byref(_lib.gpca_admix_params(*par)) if par else None, None, folds, 0, vp(q), vp(f),
                                   o if out else None, ctypes.byref(ctypes.c_double()) if err else None)
            return rc, lib.gpca_last_error(e._h).decode()

        assert step()[0] == _lib.GPCA_OK and cvf()[0] == _lib.GPCA_OK and cvf((K, 1, 0, 1e-7, 1, 1), q=Q, f=F)[0] == _lib.GPCA_OK
        neg, zero = Q.copy(), Q.copy()
        neg[4, 1] = -1e-3; zero[5] = 0
        for got, word in ((step(folds=0), "folds"), (step(folds=1), "folds"), (step(folds=65), "folds"), (step(fold=-1), "fold must"),
                          (step(fold=5), "fold must"), (step(folds=2, fold=2), "fold must"), (step(qn=None), "required"), (step(ll=None), "required"),
                          (step(hl=None), "held_loglik"), (step(nh=None), "n_held"), (step(nhet=None), "n_het_held"), (step(k=17), "K must be"),
                          (step(q=neg), "Q[4][1]"),
                          (cvf(folds=0), "folds"), (cvf(folds=1), "folds"), (cvf(folds=65), "folds"), (cvf(par=None), "required"),
                          (cvf(out=False), "out"), (cvf(err=False), "cv_error"), (cvf((17, 1, 0, 1e-7, 1, 0)), "K must be"),
                          (cvf((K, 1, 0, -1.0, 1, 0)), "tol"), (cvf((K, 1, 0, 1e-7, 1, 1)), "Q0"), (cvf((K, 1, 0, 1e-7, 1, 1), q=neg, f=F), "Q[4][1]"),
                          (cvf((K, 1, 0, 1e-7, 1, 1), q=zero, f=F), "row 5")):
            assert got[0] == _lib.GPCA_ERR_BAD_ARG and word in got[1] and "gpca_admix_" in got[1], (got, word)
        with pytest.raises(GpcaError) as ei:
            gpca.admix_cv_fold(0, 65, 4, 4)
        assert ei.value.status == _lib.GPCA_ERR_BAD_ARG and "folds" in str(ei.value)
        e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.zeros(M, np.uint8))
        each(e, _lib.GPCA_ERR_STATE, "no kept row")
    with gpca.GpcaEngine() as e:                                                         # a streamed handle
        e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), M, N, panel_rows=256, ring_slots=2, fused=False)
        e.snp_stats(gpca.QcConfig.none())
        each(e, _lib.GPCA_ERR_STATE, "panel")


def test_the_timing_record_is_its_own():
    G = make(64, 300, seed=15)
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        load(e, G)
        e.enable_timings(True)
        e.reset_timings()
        e.admix_step_holdout(*theta(64, 300, 4, seed=1500), 5, 0)
        t = e.timings()
    assert "admix_step" not in t and t["admix_step_holdout"]["launches"] == 1 and t["admix_step_holdout"]["flops"] == 12.0 * 4 * 64 * 300
