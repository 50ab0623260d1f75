"""gpca_assoc_qtl: the many-trait QTL scan (assoc_qtl.hip, gpca_assoc_qtl.cpp; gpca.h section a24), through the C ABI.

The model is gpca_assoc_linear itself, which test_gpu_assoc.py holds to derived bars and to lstsq: it is called over trait groups of
width 64 - Pc, its xb and rowinfo are collected, and liveness, r2 = (xb xb) / (sxx yy_t) and the hit set are formed in numpy f64 with the
products and the division written as in step 3 of the section.  Every output is compared with np.array_equal (NaN-aware for the best
values): hit_count, n_found, the records in (row, trait) order with their xb and r2, rowinfo, best_r2, best_row.  No tolerance enters.
yy_t is the one input of step 3 that gpca_assoc_linear does not return.  It is a host sum; the section says that a trait column is
treated on its own, so the yy of a wide call is held, bit for bit, to the yy of a one-trait call, and to numpy's restatement of the
design (test_gpu_assoc.design) within a bar: the engine's Cholesky basis departs from numpy's Householder one by at most 8 (Pc + 2)
kappa^2 e per unit-norm column (the bar test_gpu_assoc.py derives; kappa = the condition number of the centred unit-norm covariates),
which moves Y~_t by that times |Yc_t| (Yc = Y centred) and yy_t = |Y~_t|^2 by twice that times |Y~_t|; the sum of n squares adds n e yy_t:
|d yy_t| <= (16 (Pc + 2) kappa^2 sqrt(|Yc_t|^2 / yy_t) + n) e yy_t.
With r2_min = 0 every pair of a live row is a hit: those cases compare the full xb matrix with gpca_assoc_linear's, bit for bit.
The shapes cross, pairwise (tests/_combos.pairwise), N, the rows, T around every multiple of the tile and of every strip width the
GPCA_QTL_TW hook forces (64 and 128 in the first table, 256, 512 and 1024 in a second one with T up to 2 049), Pc, the storage /
precision, the missing pattern and the threshold.  The kernel has one path for all N (the calls
are staged per tile), so there is no LDS-residency threshold to straddle."""
import ctypes as C
import os

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from genomic_pca_amd._lib import GpcaError
from _combos import case_id, pairwise
from test_gpu_assoc import design

pytestmark = pytest.mark.gpu

ENGINES = {"int8": dict(storage=_lib.STORE_INT8), "2bit": dict(storage=_lib.STORE_2BIT),
           "f32": dict(storage=_lib.STORE_INT8, precision=_lib.PREC_F32_MFMA)}
VIF = 50.0
EPS = 2.0 ** -53
MISSING = -127
# T: 1, around 32 and 64 (the column block and the tile), and TW - 1, TW, TW + 1, 2 TW + 1 for the forced strip widths 64 and 128
AXES = [("N", [3, 63, 64, 65, 255, 256, 257, 1025]), ("rows", [1, 127, 128, 129, 300]),
        ("T", [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257]), ("Pc", [0, 1, 10, 63]), ("eng", ["int8", "2bit", "f32"]),
        ("miss", ["none", "one", "5 %"]), ("tw", [None, 64, 128]), ("thr", ["dense", "sparse"])]
TABLE = pairwise(AXES, seed=24)
# the wider strips the hook forces (qtl_clamp_tw: 256, 512, 1024): T = TW - 1, TW, TW + 1 (a strip edge) and 2 TW + 1 (a third strip of
# one column), over two and three row blocks, whose strips add to the same rows' hit_count; Pc <= 10 keeps the model's loop short
WIDE_AXES = [("tw", [256, 512, 1024]), ("T", ["TW-1", "TW", "TW+1", "2TW+1"]), ("rows", [129, 300]), ("N", [65, 257]), ("Pc", [0, 10]),
             ("eng", ["int8", "2bit", "f32"]), ("miss", ["none", "one", "5 %"]), ("thr", ["dense", "sparse"])]
WIDE_T = {"TW-1": lambda w: w - 1, "TW": lambda w: w, "TW+1": lambda w: w + 1, "2TW+1": lambda w: 2 * w + 1}
WIDE_TABLE = [dict(c, T=WIDE_T[c["T"]](c["tw"])) for c in pairwise(WIDE_AXES, seed=25)]


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


def make_inputs(M, N, T, Pc, seed, miss):
    """calls, traits, covariates and the include mask.  From 63 samples on sample 1 (first include word) and sample N - 1 (last word) are
    excluded and hold missing calls and extreme values.  From 5 rows and 63 samples on: row 0 has no observed call, row 2 is monomorphic
    over the included samples, row 1 is collinear with covariate 0 beyond max_vif (Pc >= 1).  miss "one": a single missing call, so
    that the e product runs in one 16-sample group of one row block only."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, M)[:, None]
    G = ((rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)).astype(np.int8)
    inc = np.ones(N, np.uint8)
    if N >= 63:
        inc[1] = 0; inc[N - 1] = 0
    Pc = max(0, min(Pc, int(inc.sum()) - 3))
    if miss == "5 %":
        G[rng.random((M, N)) < 0.05] = MISSING
    elif miss == "one":
        G[min(3, M - 1), min(37, N - 1) if N >= 63 else 0] = MISSING
    Y = rng.standard_normal((N, T))
    Cv = rng.standard_normal((N, Pc))
    special = M >= 5 and N >= 63
    if special:
        G[0, :] = MISSING
        G[2, :] = 2
        if Pc:
            o = G[1] != MISSING
            Cv[:, 0] = np.where(o, G[1], G[1][o & (inc == 1)].mean()) + 1e-7 * Cv[:, 0]
    G[:, inc == 0] = MISSING
    Y[inc == 0] = 1e30
    Cv[inc == 0] = -1e30
    return G, Y, Cv, inc, Pc, special


def load(e, G, keep=None):
    e.upload_genotypes_i8(G)
    M = G.shape[0]
    e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.ones(M, np.uint8) if keep is None else keep)


def a12(e, Y, Cv, inc, rows=None):
    """gpca_assoc_linear over trait groups of width 64 - Pc: xb [rows][T] and rowinfo"""
    T, Pc = Y.shape[1], Cv.shape[1]
    W = 64 - Pc
    xb = []
    for t0 in range(0, T, W):
        r = e.assoc_linear(Y[:, t0:t0 + W], Cv, include=inc, max_vif=VIF, rows=rows, xb=True)
        xb.append(r["xb"][:, :min(W, T - t0)])
    return np.hstack(xb), r


def model(xb, info, yy, r2_min, row0=0):
    """step 3 in numpy f64: liveness, r2, the hit set in (row, trait) order, the counts, the best values"""
    nobs, xx, sxx = info["n_obs"], info["xx"], info["sxx"]
    with np.errstate(all="ignore"):
        live = ~((nobs == 0) | ~(xx > 0.0) | (sxx * VIF < xx))
        r2 = (xb * xb) / (sxx[:, None] * yy[None, :])
        hit = live[:, None] & (r2 >= r2_min)
    ri, ti = np.nonzero(hit)                              # row-major: ascending (row, trait)
    T = xb.shape[1]
    best_r2 = np.full(T, np.nan)
    best_row = np.full(T, -1, np.int64)
    if live.any():
        lr = np.flatnonzero(live)
        sub = r2[lr]
        best_r2 = sub.max(0)
        best_row = lr[np.argmax(sub == best_r2[None, :], 0)].astype(np.int64) + row0      # the first (smallest) row that attains it
    return dict(live=live, r2=r2, hit_count=hit.sum(1).astype(np.uint32), n_found=int(hit.sum()), rows=(ri + row0).astype(np.uint32),
                traits=ti.astype(np.uint32), xb=xb[ri, ti], r2_hits=r2[ri, ti], best_r2=best_r2, best_row=best_row)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def check(q, m, info):
    for k in ("n_obs", "a1_freq", "xx", "sxx"):
        assert same(q[k], info[k]), k
    assert np.array_equal(q["hit_count"], m["hit_count"]) and q["n_found"] == m["n_found"]
    assert np.array_equal(q["rows"], m["rows"]) and np.array_equal(q["traits"], m["traits"])
    assert np.array_equal(q["xb"], m["xb"]) and np.array_equal(q["r2"], m["r2_hits"])
    assert same(q["best_r2"], m["best_r2"]) and np.array_equal(q["best_row"], m["best_row"])


def sparse_threshold(r2, live):
    """a threshold that keeps about 2 % of the live pairs (at least one): the r2 of a pair itself, so the edge r2 = r2_min is met"""
    v = np.sort(r2[live].ravel())
    return min(float(v[int(0.98 * (v.size - 1))]), 1.0) if v.size else 0.5


# ------------------------------------------------------------------------------------------------ the crossed edge shapes
@pytest.mark.parametrize("c", TABLE, ids=case_id)
def test_scan_equals_assoc_linear(c, tw_env):
    scan_case(c, 1000 + TABLE.index(c), tw_env)


@pytest.mark.parametrize("c", WIDE_TABLE, ids=case_id)
def test_scan_equals_assoc_linear_at_wide_strips(c, tw_env):
    scan_case(c, 2000 + WIDE_TABLE.index(c), tw_env)


def test_wide_table_holds_every_strip_edge():
    assert {(c["tw"], c["T"]) for c in WIDE_TABLE} == {(w, t) for w in (256, 512, 1024) for t in (w - 1, w, w + 1, 2 * w + 1)}


def scan_case(c, seed, tw_env):
    M = c["rows"]
    G, Y, Cv, inc, Pc, special = make_inputs(M, c["N"], c["T"], c["Pc"], seed=seed, miss=c["miss"])
    tw_env(c["tw"])
    with gpca.GpcaEngine(**ENGINES[c["eng"]]) as e:
        load(e, G)
        xb, info = a12(e, Y, Cv, inc)
        q0 = e.assoc_qtl(Y, Cv, include=inc, max_vif=VIF, r2_min=0.0)
        yy = q0["yy"]
        live = model(xb, info, yy, 0.0)["live"]
        thr = 0.0 if c["thr"] == "dense" else sparse_threshold(model(xb, info, yy, 0.0)["r2"], live)
        q = q0 if thr == 0.0 else e.assoc_qtl(Y, Cv, include=inc, max_vif=VIF, r2_min=thr)
        one = e.assoc_qtl(Y[:, -1:], Cv, include=inc, max_vif=VIF, r2_min=1.0, best=False)
    m = model(xb, info, yy, thr)
    check(q, m, info)
    if thr == 0.0:                                        # dense: the whole xb matrix of the live rows, bit for bit
        assert q["n_found"] == int(live.sum()) * c["T"]
        assert np.array_equal(q["xb"].reshape(-1, c["T"]), xb[live])
    else:
        assert q["n_found"] >= 1 or not live.any()
    # yy: a trait on its own gives the same bits; numpy's design within the docstring's bar
    assert one["yy"][0] == yy[-1] and q["df"] == int(inc.sum()) - Pc - 2
    _, yy_ref, df, kappa = design(Y, Cv, inc)
    sb = inc.astype(bool)
    yyc = ((Y[sb] - Y[sb].mean(0)) ** 2).sum(0)
    bar = (16 * (Pc + 2) * kappa ** 2 * np.sqrt(yyc / yy_ref) + sb.sum()) * EPS * yy_ref
    print("yy: max err / bar", np.max(np.abs(yy - yy_ref) / bar), "kappa", kappa)
    assert np.all(np.abs(yy - yy_ref) <= bar)
    if special:
        assert not live[0] and not live[2] and q["hit_count"][0] == 0 and q["hit_count"][2] == 0
        if Pc:
            assert not live[1] and q["hit_count"][1] == 0


def test_tiny_sample_counts():
    G = np.array([[0, 1, 2], [2, 1, 0], [1, 1, 2]], np.int8)
    rng = np.random.default_rng(3)
    for N in (1, 2):
        with gpca.GpcaEngine() as e:
            load(e, G[:, :N].copy())
            with pytest.raises(GpcaError) as ei:
                e.assoc_qtl(rng.standard_normal((N, 2)), r2_min=0.0)
            assert ei.value.status == _lib.GPCA_ERR_BAD_ARG and "df" in str(ei.value)


# ------------------------------------------------------------------------------------------------ threshold, capacity, bands
@pytest.fixture(scope="module")
def mid():
    """300 rows x 257 samples x 200 traits, 5 % missing, 3 covariates: inputs, gpca_assoc_linear's xb and rowinfo, yy"""
    G, Y, Cv, inc, Pc, _ = make_inputs(300, 257, 200, 3, seed=77, miss="5 %")
    with gpca.GpcaEngine() as e:
        load(e, G)
        xb, info = a12(e, Y, Cv, inc)
        yy = e.assoc_qtl(Y, Cv, include=inc, max_vif=VIF, r2_min=1.0)["yy"]
    return dict(G=G, Y=Y, C=Cv, inc=inc, xb=xb, info=info, yy=yy)


def test_threshold_edges(mid):
    m0 = model(mid["xb"], mid["info"], mid["yy"], 0.0)
    i, t = 150, 77
    assert m0["live"][i]
    r2 = float(m0["r2"][i, t])
    with gpca.GpcaEngine() as e:
        load(e, mid["G"])
        at = e.assoc_qtl(mid["Y"], mid["C"], include=mid["inc"], max_vif=VIF, r2_min=r2)
        above = e.assoc_qtl(mid["Y"], mid["C"], include=mid["inc"], max_vif=VIF, r2_min=float(np.nextafter(r2, 2.0)))
        top = e.assoc_qtl(mid["Y"], mid["C"], include=mid["inc"], max_vif=VIF, r2_min=1.0)
    pairs = lambda q: set(zip(q["rows"].tolist(), q["traits"].tolist()))
    assert (i, t) in pairs(at) and (i, t) not in pairs(above)
    assert at["n_found"] == above["n_found"] + int((m0["r2"][m0["live"]] == r2).sum())
    check(at, model(mid["xb"], mid["info"], mid["yy"], r2), mid["info"])
    check(top, model(mid["xb"], mid["info"], mid["yy"], 1.0), mid["info"])
    assert top["n_found"] == 0


def test_t_min_maps_to_r2(mid):
    with gpca.GpcaEngine() as e:
        load(e, mid["G"])
        q = e.assoc_qtl(mid["Y"], mid["C"], include=mid["inc"], max_vif=VIF, t_min=3.0)
        with pytest.raises(ValueError):
            e.assoc_qtl(mid["Y"], mid["C"], r2_min=0.1, t_min=3.0)
        with pytest.raises(ValueError):
            e.assoc_qtl(mid["Y"], mid["C"])
    df = q["df"]
    assert q["r2_min"] == 9.0 / (9.0 + df)
    check(q, model(mid["xb"], mid["info"], mid["yy"], q["r2_min"]), mid["info"])
    assert q["n_found"] > 0
    # the host rule on the hits: |t| >= t_min up to the rounding of the map (t^2 = df r2 / (1 - r2))
    st = gpca.qtl_stats(q["xb"], mid["info"]["sxx"][q["rows"]], q["yy"][q["traits"]], df)
    assert np.all(np.abs(st[:, 2]) >= 3.0 * (1 - 1e-12))


def test_capacity(mid):
    thr = sparse_threshold(model(mid["xb"], mid["info"], mid["yy"], 0.0)["r2"], model(mid["xb"], mid["info"], mid["yy"], 0.0)["live"])
    m = model(mid["xb"], mid["info"], mid["yy"], thr)
    nf = m["n_found"]
    assert nf > 100
    with gpca.GpcaEngine() as e:
        load(e, mid["G"])
        for cap in (nf, nf - 1, 0):
            q = e.assoc_qtl(mid["Y"], mid["C"], include=mid["inc"], max_vif=VIF, r2_min=thr, cap=cap)      # (GPCA_OK: no exception)
            assert q["n_found"] == nf and np.array_equal(q["hit_count"], m["hit_count"])
            assert same(q["best_r2"], m["best_r2"]) and np.array_equal(q["best_row"], m["best_row"])
            if cap == nf:
                check(q, m, mid["info"])
            else:
                assert q["rows"] is None


@pytest.mark.parametrize("cuts", [(0, 70, 300), (0, 50, 100, 300)])
def test_bands_inside_a_row_block(mid, cuts):
    full = model(mid["xb"], mid["info"], mid["yy"], 0.0)
    thr = sparse_threshold(full["r2"], full["live"])
    m = model(mid["xb"], mid["info"], mid["yy"], thr)
    parts = []
    with gpca.GpcaEngine(storage=_lib.STORE_2BIT) as e:
        load(e, mid["G"])
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            parts.append(e.assoc_qtl(mid["Y"], mid["C"], include=mid["inc"], max_vif=VIF, r2_min=thr, rows=(r0, r1)))
    for k, mk in (("rows", "rows"), ("traits", "traits"), ("xb", "xb"), ("r2", "r2_hits"), ("hit_count", "hit_count")):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), m[mk]), k
    # the running best over the bands: a later band wins only with a strictly larger r2
    b2, bw = np.full(200, np.nan), np.full(200, -1, np.int64)
    for p in parts:
        with np.errstate(invalid="ignore"):
            take = (p["best_row"] >= 0) & ((bw < 0) | (p["best_r2"] > b2))
        b2, bw = np.where(take, p["best_r2"], b2), np.where(take, p["best_row"], bw)
    assert same(b2, m["best_r2"]) and np.array_equal(bw, m["best_row"])


def test_best_tie_goes_to_the_lower_row():
    """rows 3 and 200 (another row block) are the same SNP and trait 0 follows it: both rows attain the trait's largest r2, bit for
    bit, and the best row is the lower one"""
    G, Y, Cv, inc, Pc, _ = make_inputs(300, 130, 70, 2, seed=5, miss="none")
    G[200] = G[3]
    Y[:, 0] = G[3] + 0.1 * Y[:, 0]
    Y[inc == 0] = 1e30
    with gpca.GpcaEngine() as e:
        load(e, G)
        xb, info = a12(e, Y, Cv, inc)
        q = e.assoc_qtl(Y, Cv, include=inc, max_vif=VIF, r2_min=0.5)
    m = model(xb, info, q["yy"], 0.5)
    check(q, m, info)
    assert q["best_row"][0] == 3 and m["r2"][3, 0] == m["r2"][200, 0]


def test_repeatable_with_many_hits(tw_env, monkeypatch):
    """several thousand hits from many workgroups (5 row blocks x 9 strips of 64): two calls give the same arrays, whatever the order in
    which the waves took their places in the record buffer; so does a third with another strip width and the host step on one thread"""
    G, Y, Cv, inc, Pc, _ = make_inputs(600, 200, 520, 4, seed=9, miss="5 %")
    tw_env(64)
    with gpca.GpcaEngine() as e:
        load(e, G)
        a = e.assoc_qtl(Y, Cv, include=inc, max_vif=VIF, t_min=2.0)
        b = e.assoc_qtl(Y, Cv, include=inc, max_vif=VIF, t_min=2.0)
        tw_env(1024)
        monkeypatch.setenv("GPCA_DESIGN_THREADS", "1")               # (the host step on one thread: 520 traits go to 4 otherwise)
        c = e.assoc_qtl(Y, Cv, include=inc, max_vif=VIF, t_min=2.0)
        xb, info = a12(e, Y, Cv, inc)
    assert a["n_found"] > 5000
    for k in ("hit_count", "rows", "traits", "xb", "r2", "best_r2", "best_row", "yy", "sxx"):
        assert same(a[k], b[k]) and same(a[k], c[k]), k
    check(a, model(xb, info, a["yy"], a["r2_min"]), info)


def test_planted_signal():
    rng = np.random.default_rng(11)
    G, Y, Cv, inc, Pc, _ = make_inputs(400, 300, 90, 2, seed=21, miss="5 %")
    trait = 41
    snp = 5 + int(np.argmax(np.where(G == MISSING, 0, G).astype(np.float64).var(1)[5:]))          # a common SNP: t is about 10
    s = inc == 1
    g = np.where(G[snp] == MISSING, 0, G[snp]).astype(np.float64)
    Y[s, trait] = 0.8 * g[s] + rng.standard_normal(int(s.sum()))
    with gpca.GpcaEngine() as e:
        load(e, G)
        q = e.assoc_qtl(Y, Cv, include=inc, max_vif=VIF, t_min=6.0)
        r = e.assoc_linear(Y[:, trait:trait + 1], Cv, include=inc, max_vif=VIF)
    assert q["best_row"][trait] == snp
    k = np.flatnonzero((q["rows"] == snp) & (q["traits"] == trait))
    assert k.size == 1
    st = gpca.qtl_stats(q["xb"][k], q["sxx"][snp], q["yy"][trait], q["df"])[0]
    t12 = r["t"][snp, 0]
    # the same three f64 operations on the same xb, sxx and yy, on the host and on the device: a few roundings apart at most
    assert abs(st[2] - t12) <= 8 * EPS * abs(t12) and abs(t12) > 6.0
    assert abs(st[0] - r["beta"][snp, 0]) <= 8 * EPS * abs(st[0])


# ------------------------------------------------------------------------------------------------ errors
def test_errors():
    rng = np.random.default_rng(2)
    M, N = 40, 50
    G = rng.integers(0, 3, (M, N)).astype(np.int8)
    Y, Cv = rng.standard_normal((N, 70)), rng.standard_normal((N, 3))
    BA, ST = _lib.GPCA_ERR_BAD_ARG, _lib.GPCA_ERR_STATE

    def err(e, Y, Cv, **kw):
        kw.setdefault("r2_min", 0.5)
        with pytest.raises(GpcaError) as ei:
            e.assoc_qtl(Y, Cv, **kw)
        return ei.value.status, str(ei.value)

    with gpca.GpcaEngine() as e:
        e.upload_genotypes_i8(G)
        assert err(e, Y, Cv)[0] == ST                                                    # no standardisation
        load(e, G, np.zeros(M, np.uint8))
        assert err(e, Y, Cv)[0] == ST                                                    # K = 0
        load(e, G)
        assert err(e, np.zeros((N, 0)), Cv)[0] == BA                                     # T = 0
        assert err(e, Y, rng.standard_normal((N, 64)))[0] == BA                          # Pc > 63
        for bad in (-0.1, 1.0000001, float("nan")):
            assert err(e, Y, Cv, r2_min=bad)[0] == BA
        assert err(e, Y, Cv, cap=-1)[0] == BA
        assert err(e, Y, Cv, max_vif=0.5)[0] == BA
        assert err(e, Y, Cv, rows=(0, M + 1))[0] == BA
        Yb = Y.copy(); Yb[7, 66] = np.inf
        assert err(e, Yb, Cv)[0] == BA and "Y[7][66]" in err(e, Yb, Cv)[1]
        inc = np.ones(N, np.uint8); inc[7] = 0
        assert e.assoc_qtl(Yb, Cv, include=inc, r2_min=0.5)["n_found"] >= 0              # not finite, but excluded
        Cb = Cv.copy(); Cb[3, 1] = np.nan
        assert err(e, Y, Cb)[0] == BA
        few = np.zeros(N, np.uint8); few[:5] = 1
        assert "df" in err(e, Y, Cv, include=few)[1]                                     # n - Pc - 2 = 0
        Cc = Cv.copy(); Cc[:, 2] = Cc[:, 0] - 2 * Cc[:, 1]
        assert "collinear" in err(e, Y, Cc)[1]
        Yc = Y.copy(); Yc[:, 65] = 3.0
        st, msg = err(e, Yc, Cv)
        assert st == BA and "trait 65" in msg
        # the pointer rules, through the C ABI itself
        lib = _lib.load()
        Yv, Cvv = np.ascontiguousarray(Y), np.ascontiguousarray(Cv)
        hc, nf = np.zeros(M, np.uint32), C.c_int64(0)
        b2, bw = np.zeros(70), np.zeros(70, np.int64)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        call = lambda hcp, nfp, b2p, bwp: lib.gpca_assoc_qtl(e._h, vp(Yv), 70, vp(Cvv), 3, None, 50.0, 0.5, 0, M, None, None, hcp, None, None, 0,
                                                            nfp, b2p, bwp)
        assert call(vp(hc), C.byref(nf), vp(b2), vp(bw)) == _lib.GPCA_OK
        assert call(None, C.byref(nf), vp(b2), vp(bw)) == BA
        assert call(vp(hc), None, vp(b2), vp(bw)) == BA
        assert call(vp(hc), C.byref(nf), vp(b2), None) == BA and call(vp(hc), C.byref(nf), None, vp(bw)) == BA
        assert call(vp(hc), C.byref(nf), None, None) == _lib.GPCA_OK
        hi, hv = np.zeros((8, 2), np.uint32), np.zeros((8, 2))
        capped = lambda hip, hvp: lib.gpca_assoc_qtl(e._h, vp(Yv), 70, vp(Cvv), 3, None, 50.0, 0.5, 0, M, None, None, vp(hc), hip, hvp, 8,
                                                    C.byref(nf), None, None)
        assert capped(vp(hi), vp(hv)) == _lib.GPCA_OK                                    # cap > 0 needs both record buffers
        assert capped(None, vp(hv)) == BA and capped(vp(hi), None) == BA and capped(None, None) == BA
        Gb = G.copy(); Gb[17, 9] = 3
        load(e, Gb)
        st, msg = err(e, Y, Cv)
        assert st == _lib.GPCA_ERR_INVALID_GENOTYPE and "row 17" in msg
        assert e.assoc_qtl(Y, Cv, r2_min=0.5, rows=(0, 17))["n_found"] >= 0              # a band that does not read the row
    with gpca.GpcaEngine() as e:                                                         # a streamed handle
        e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), M, N, panel_rows=256, ring_slots=2, fused=False)
        e.snp_stats(gpca.QcConfig.none())
        st, msg = err(e, Y, Cv)
        assert st == ST and "panel" in msg
    with gpca.GpcaEngine() as e:                                                         # a hooked (row-sharded) handle
        e.upload_genotypes_i8(G[:20].copy())
        e.set_allreduce_hook(lambda buf: None, 2, 0, 0)
        e.set_standardization(np.ones(20, np.float32), np.ones(20, np.float32), np.ones(20, np.uint8))
        st, msg = err(e, Y, Cv)
        assert st == ST and "shard" in msg
