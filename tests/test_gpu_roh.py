"""gpca_roh (roh.hip, gpca_roh.cpp; include/gpca.h section a20) through the C ABI against a numpy restatement of the rule.

Everything is an exact integer, so every comparison is ``array_equal``: the records ``segs``, ``seg_count`` and ``n_found``.  The model
(``model``) follows a20's steps as they are written -- per domain, cumulative sums of the het and missing calls give every window's
counts, a cumulative sum of the hits gives every row's hits among its covering windows, and the runs are the maximal stretches of
in-ROH rows cut before the rows with bit 1 -- and shares no arithmetic with the kernels (no running counts, no hit history, no
splits).  Every case first asserts on the MODEL's output that it can bite: that there are records at all and, where splits are forced,
that a record's first and last row lie in different splits.

Shapes are the smallest that reach the edges: windows 1, 2, 5, 50, 63, 64 with domains of W - 1, W, W + 1, 2 W - 1 and 2 W rows; the
sample counts around the thread's 16 samples and the wave's 1 024; the keep masks of tests/_edges.py; forced split counts 1, 2, 3, 7 and
rows; runs that meet at a split boundary; a break at every row in turn; the threshold at equality; the limits of H, M, max_het and
min_snp; short, exact and empty record buffers; bands cut at domain starts and inside a domain; both storages and an f32-precision
handle; and a20's refusals."""
import ctypes

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from genomic_pca_amd._lib import GpcaError

from _edges import edge_keeps

pytestmark = pytest.mark.gpu

STORES = {"int8": _lib.STORE_INT8, "2bit": _lib.STORE_2BIT}
MISSING = -127
DEFAULTS = dict(W=50, H=1, M=5, num=1, den=20, min_snp=100, max_het=-1)


def P(**kw):
    d = dict(DEFAULTS)
    d.update(kw)
    return d


def make(K, N, het, miss, seed):
    """independent calls: a share `het` of 1, a share `miss` missing, the rest split evenly between 0 and 2"""
    rng = np.random.default_rng(seed)
    u = rng.random((K, N))
    G = np.where(rng.random((K, N)) < 0.5, 0, 2).astype(np.int8)
    G[u < het] = 1
    G[(u >= het) & (u < het + miss)] = MISSING
    return G


def breaks(K, dom=(), cut=()):
    """brk [K]: 3 at row 0 and at the rows of `dom`, 2 at the rows of `cut`"""
    b = np.zeros(K, np.uint8)
    b[0] = 3
    for j in dom:
        b[j] = 3
    for j in cut:
        b[j] |= 2
    return b


def model(G, brk, p, keep=None, rows=None):
    """(segs uint32 [n][5], seg_count uint32 [N]) of the kept rows [rows[0], rows[1]) of G, as a20 states the rule"""
    W, H, M, num, den = p["W"], p["H"], p["M"], p["num"], p["den"]
    Gk = G if keep is None else G[np.asarray(keep) != 0]
    r0, r1 = (0, Gk.shape[0]) if rows is None else rows
    band = Gk[r0:r1]
    K, N = band.shape
    if K == 0:
        return np.zeros((0, 5), np.uint32), np.zeros(N, np.uint32)
    b = np.asarray(brk, np.uint8).copy()
    b[0] = 3
    het, mis = (band == 1), (band == MISSING)
    inroh = np.zeros((K, N), bool)
    starts = [j for j in range(K) if b[j] & 1] + [K]
    for d0, d1 in zip(starts[:-1], starts[1:]):
        L = d1 - d0
        if L < W:
            continue
        zero = np.zeros((1, N), np.int64)
        ch = np.concatenate([zero, np.cumsum(het[d0:d1], 0)])
        cm = np.concatenate([zero, np.cumsum(mis[d0:d1], 0)])
        hit = ((ch[W:] - ch[:-W]) <= H) & ((cm[W:] - cm[:-W]) <= M)              # [L - W + 1][N]: window s = rows s .. s + W - 1
        chit = np.concatenate([zero, np.cumsum(hit, 0)])
        for j in range(L):
            lo, hi = max(0, j - W + 1), min(j, L - W)
            cov = hi - lo + 1
            hits = chit[hi + 1] - chit[lo]
            inroh[d0 + j] = (hits * den >= num * cov) if cov > 0 else False
    cut = (b & 2) != 0                                                           # no run continues INTO the row
    prev = np.concatenate([np.zeros((1, N), bool), inroh[:-1]])
    nxt = np.concatenate([inroh[1:], np.zeros((1, N), bool)])
    cutn = np.concatenate([cut[1:], [True]])
    first = inroh & (~prev | cut[:, None])
    last = inroh & (~nxt | cutn[:, None])
    sf, jf = np.nonzero(first.T)                                                 # ascending (sample, row)
    sl, jl = np.nonzero(last.T)
    assert np.array_equal(sf, sl) and np.all(jl >= jf)
    cumh = np.concatenate([np.zeros((1, N), np.int64), np.cumsum(het, 0)])
    cumm = np.concatenate([np.zeros((1, N), np.int64), np.cumsum(mis, 0)])
    nh = cumh[jl + 1, sf] - cumh[jf, sf]
    nm = cumm[jl + 1, sf] - cumm[jf, sf]
    rep = (jl - jf + 1 >= p["min_snp"]) & ((p["max_het"] < 0) | (nh <= p["max_het"]))
    segs = np.stack([sf, r0 + jf, r0 + jl, nh, nm], 1)[rep].astype(np.uint32)
    return segs.reshape(-1, 5), np.bincount(sf[rep], minlength=N).astype(np.uint32)


def load(e, G, keep=None):
    e.upload_genotypes_i8(G)
    M = G.shape[0]
    e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), np.ones(M, np.uint8) if keep is None else keep)


def call(e, brk, p, rows=None):
    return e.roh(brk, window_snp=p["W"], window_het=p["H"], window_missing=p["M"], window_threshold=(p["num"], p["den"]),
                 min_snp=p["min_snp"], max_het=None if p["max_het"] < 0 else p["max_het"], rows=rows)


def check(e, G, brk, p, keep=None, rows=None, what=None):
    want, wcount = model(G, brk, p, keep, rows)
    segs, count = call(e, brk, p, rows)
    assert segs.dtype == np.uint32 and count.dtype == np.uint32 and segs.shape[1:] == (5,) and count.shape == (G.shape[1],)
    assert np.array_equal(count, wcount), what
    assert segs.shape == want.shape and np.array_equal(segs, want), what
    return want


def crossing(segs, K, splits):
    """the records whose first and last row lie in different splits of a K-row band forced to `splits` splits"""
    s = max(1, min(splits, K))
    per = (K + s - 1) // s
    return int(np.sum(segs[:, 1] // per != segs[:, 2] // per))


#        K    N     W  H  M  num den min_snp het   miss  a record must cross a split
TABLE = [(200, 33, 5, 0, 0, 1, 1, 1, 0.15, 0.02, True),
         (200, 33, 5, 1, 1, 1, 20, 8, 0.30, 0.05, True),
         (600, 17, 50, 1, 5, 1, 20, 100, 0.02, 0.02, True),
         (300, 1025, 8, 1, 1, 1, 4, 10, 0.25, 0.03, True),
         (130, 16, 64, 1, 5, 1, 20, 64, 0.01, 0.01, False),
         (70, 40, 3, 0, 1, 1, 2, 2, 0.30, 0.10, False)]


@pytest.mark.parametrize("store", sorted(STORES))
@pytest.mark.parametrize("case", range(len(TABLE)))
def test_random_calls_with_two_breaks(case, store, monkeypatch):
    K, N, W, H, M, num, den, min_snp, het, miss, cross = TABLE[case]
    G = make(K, N, het, miss, seed=10 + case)
    brk = breaks(K, dom=[K // 3], cut=[K // 2])
    p = P(W=W, H=H, M=M, num=num, den=den, min_snp=min_snp)
    want, _ = model(G, brk, p)
    splits = (K + 63) // 64
    assert len(want) > 0
    if cross:
        assert crossing(want, K, splits) > 0
    for s in (None, 1, splits):                                                      # (one split: a run of 300 rows passes the 255-row flush)
        if s is None:
            monkeypatch.delenv("GPCA_ROH_SPLITS", raising=False)
        else:
            monkeypatch.setenv("GPCA_ROH_SPLITS", str(s))
        with gpca.GpcaEngine(storage=STORES[store]) as e:
            load(e, G)
            check(e, G, brk, p, what=(case, s))


@pytest.mark.parametrize("W", [1, 2, 5, 50, 63, 64])
def test_windows_and_domain_lengths(W, monkeypatch):
    """domains of W - 1 (no window: no record), W, W + 1, 2 W - 1 and 2 W rows in one band, at one split and at several"""
    lens = [L for L in (W - 1, W, W + 1, 2 * W - 1, 2 * W) if L > 0]
    K, N = sum(lens), 19
    G = make(K, N, 0.03 if W > 5 else 0.25, 0.02, seed=100 + W)
    dom = list(np.cumsum(lens)[:-1])
    brk = breaks(K, dom=dom)
    p = P(W=W, H=1 if W > 1 else 0, M=min(W, 5) if W > 1 else 0, num=1, den=4, min_snp=1)
    want, _ = model(G, brk, p)
    assert len(want) > 0
    if W > 1:
        assert not np.any(want[:, 2] < W - 1)                                        # the first domain (W - 1 rows) holds no record
    for s in (1, 3, K):
        monkeypatch.setenv("GPCA_ROH_SPLITS", str(s))
        for store in sorted(STORES):
            with gpca.GpcaEngine(storage=STORES[store]) as e:
                load(e, G)
                check(e, G, brk, p, what=(W, s, store))


@pytest.mark.parametrize("store", sorted(STORES))
def test_sample_counts(store):
    K, W = 90, 6
    brk = breaks(K, dom=[31], cut=[60])
    p = P(W=W, H=1, M=1, num=1, den=3, min_snp=4)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        for N in (1, 15, 16, 17, 1023, 1024, 1025):
            G = make(K, N, 0.2, 0.04, seed=200 + N)
            G[:, N - 1] = 0                                                          # the last sample holds records
            load(e, G)
            want = check(e, G, brk, p, what=N)
            assert [tuple(int(v) for v in r[1:3]) for r in want if r[0] == N - 1] == [(0, 30), (31, 59), (60, 89)]


@pytest.mark.parametrize("store", sorted(STORES))
def test_keep_masks(store):
    M, N = 257, 40
    G = make(M, N, 0.2, 0.03, seed=300)
    rng = np.random.default_rng(301)
    masks = edge_keeps(M) + [("random half", (rng.random(M) < 0.5).astype(np.uint8))]
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        for name, keep in masks:
            K = int(keep.sum())
            load(e, G, keep)
            p = P(W=min(4, K), H=1, M=1, num=1, den=2, min_snp=1)
            brk = breaks(K, dom=[K // 2] if K > 1 else [])
            want = check(e, G, brk, p, keep=keep, what=name)
            assert len(want) > 0


def test_every_forced_split_gives_the_same_bits(monkeypatch):
    K, N = 300, 70
    G = make(K, N, 0.08, 0.03, seed=400)
    G[:, 5] = 0                                                                      # one run through every split
    brk = breaks(K)
    p = P(W=10, H=1, M=2, num=1, den=5, min_snp=12)
    want, wcount = model(G, brk, p)
    assert any(tuple(r[:3]) == (5, 0, K - 1) for r in want)
    for s in (1, 2, 3, 7, K):
        if s > 1:
            assert crossing(want, K, s) > 0
        monkeypatch.setenv("GPCA_ROH_SPLITS", str(s))
        for store in sorted(STORES):
            with gpca.GpcaEngine(storage=STORES[store]) as e:
                load(e, G)
                segs, count = call(e, brk, p)
                assert np.array_equal(segs, want) and np.array_equal(count, wcount), (s, store)


@pytest.mark.parametrize("between", ["break", "het"])
def test_runs_that_meet_at_a_split_boundary(between, monkeypatch):
    """4 splits of 25 rows: one run ends on row 49, the last of split 1, and the next begins on row 50 (a bit-1 break at row 50), or the
    two are parted by the single het row 50 and the next begins on row 51; W = 1 makes a row in-ROH iff it is not het"""
    K, N = 100, 18
    G = np.zeros((K, N), np.int8)
    G[20, :] = 1
    G[80, :] = 1
    p = P(W=1, H=0, M=1, num=1, den=1, min_snp=1)
    if between == "break":
        brk = breaks(K, cut=[50])
        exp = [(21, 49), (50, 79)]
    else:
        G[50, :] = 1
        G[49, 3] = MISSING
        brk = breaks(K)
        exp = [(21, 49), (51, 79)]
    want, _ = model(G, brk, p)
    got = {(int(r[1]), int(r[2])) for r in want if r[0] == 3}
    assert set(exp) <= got
    monkeypatch.setenv("GPCA_ROH_SPLITS", "4")
    for store in sorted(STORES):
        with gpca.GpcaEngine(storage=STORES[store]) as e:
            load(e, G)
            check(e, G, brk, p, what=(between, store))


@pytest.mark.parametrize("bit", [2, 3])
def test_a_break_at_every_row_in_turn(bit, monkeypatch):
    K, N = 40, 21
    G = make(K, N, 0.1, 0.03, seed=500)
    p = P(W=4, H=1, M=1, num=1, den=2, min_snp=2)
    monkeypatch.setenv("GPCA_ROH_SPLITS", "3")
    seen = set()
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        load(e, G)
        for j in range(K):
            brk = breaks(K)
            brk[j] = 3 if j == 0 else bit
            want = check(e, G, brk, p, what=(bit, j))
            assert len(want) > 0
            seen.add(want.tobytes())
    assert len(seen) > 10                                                            # the break moves the records


def test_the_threshold_at_equality_and_at_its_ends():
    """W = 20 in one domain of 60 rows; sample 0 has exactly one hit window (window 20) among the 20 that cover rows 20 .. 39"""
    K, N, W = 60, 16, 20
    G = np.zeros((K, N), np.int8)
    G[19, 0] = 1                                                                     # windows 0 .. 19 hold it
    G[40, 0] = 1                                                                     # windows 21 .. 40 hold it: window 20 alone is clean
    G[:, 1] = 0
    G[10, 2] = 1
    brk = breaks(K)
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        load(e, G)
        p = P(W=W, H=0, M=0, num=1, den=20, min_snp=1)
        want = check(e, G, brk, p)
        assert (0, 20, 39, 0, 0) in [tuple(int(v) for v in r) for r in want]          # hits 1 x den 20 = num 1 x cov 20
        want = check(e, G, brk, P(W=W, H=0, M=0, num=2, den=39, min_snp=1))          # a hair above 1/20: gone
        assert not np.any(want[:, 0] == 0)
        want = check(e, G, brk, P(W=W, H=0, M=0, num=1, den=1, min_snp=1))           # every covering window must hit
        assert (2, 30, 59, 0, 0) in [tuple(int(v) for v in r) for r in want] and not np.any(want[:, 0] == 0)
        want = check(e, G, brk, P(W=W, H=0, M=0, num=0, den=1, min_snp=1))           # every covered row is in
        assert np.array_equal(want[:3], np.array([[0, 0, 59, 2, 0], [1, 0, 59, 0, 0], [2, 0, 59, 1, 0]], np.uint32))
        want = check(e, G, breaks(K, dom=[45]), P(W=W, H=0, M=0, num=0, den=1, min_snp=1))   # ... but not a row without a window
        assert want[:, 2].max() == 44


def test_limits():
    K, N, W = 120, 33, 6
    G = make(K, N, 0.12, 0.06, seed=600)
    brk = breaks(K, dom=[50])
    with gpca.GpcaEngine(storage=_lib.STORE_2BIT) as e:
        load(e, G)
        for H, M in ((0, 0), (0, W), (W, 0), (W, W), (1, 2)):
            want = check(e, G, brk, P(W=W, H=H, M=M, num=1, den=2, min_snp=3), what=(H, M))
            assert len(want) > 0
        p = P(W=W, H=1, M=2, num=1, den=2, min_snp=3)
        free = check(e, G, brk, p)
        none = check(e, G, brk, dict(p, max_het=0))
        assert 0 < len(none) < len(free) and not none[:, 3].any() and free[:, 3].any()
        r = free[len(free) // 2]
        n = int(r[2] - r[1] + 1)
        at = check(e, G, brk, dict(p, min_snp=n))
        above = check(e, G, brk, dict(p, min_snp=n + 1))
        assert any(np.array_equal(r, x) for x in at) and not any(np.array_equal(r, x) for x in above)


def test_buffer_handling():
    K, N = 150, 45
    G = make(K, N, 0.2, 0.03, seed=700)
    brk = breaks(K, dom=[70])
    p = P(W=5, H=1, M=1, num=1, den=2, min_snp=3)
    want, wcount = model(G, brk, p)
    nf = len(want)
    assert nf > 10
    lib = _lib.load()
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    par = _lib.gpca_roh_params(p["W"], p["H"], p["M"], p["num"], p["den"], p["min_snp"], p["max_het"])
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        load(e, G)
        for cap in (0, 1, nf - 1, nf, nf + 7):
            segs = np.full((max(cap, 1), 5), 0xdeadbeef, np.uint32)
            count = np.full(N, 77, np.uint32)
            found = ctypes.c_int64(-1)
            rc = lib.gpca_roh(e._h, 0, K, vp(brk), ctypes.byref(par), vp(count), vp(segs) if cap else None, cap, ctypes.byref(found))
            assert rc == _lib.GPCA_OK, lib.gpca_last_error(e._h).decode()
            assert found.value == nf and np.array_equal(count, wcount), cap
            got = min(cap, nf)
            assert np.array_equal(segs[:got], want[:got]), cap
            assert np.all(segs[got:] == 0xdeadbeef), cap                             # nothing is written behind the records
        segs, count = e.roh(brk, window_snp=5, window_het=1, window_missing=1, window_threshold=0.5, min_snp=3)
        assert np.array_equal(segs, want) and np.array_equal(count, wcount)
    # the wrapper comes back with a larger buffer: more records than its first buffer of max(4 N, 1024)
    G2 = np.zeros((4000, 2), np.int8)
    G2[1::3] = 1
    b2 = breaks(4000)
    p2 = P(W=1, H=0, M=0, num=1, den=1, min_snp=1)
    w2, c2 = model(G2, b2, p2)
    assert len(w2) > 1024
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        load(e, G2)
        check(e, G2, b2, p2)


def test_bands():
    """three domains: every cut at domain starts gives the records of the full call; a band that starts inside a domain gives what the
    rule says for brk[row0] = 3"""
    K, N = 180, 37
    d1, d2 = 55, 120
    G = make(K, N, 0.12, 0.03, seed=800)
    brk = breaks(K, dom=[d1, d2], cut=[30, 90])
    p = P(W=7, H=1, M=1, num=1, den=3, min_snp=5)
    want, wcount = model(G, brk, p)
    assert len(want) > 0
    with gpca.GpcaEngine(storage=_lib.STORE_2BIT) as e:
        load(e, G)
        check(e, G, brk, p)
        for cuts in ([0, d1, K], [0, d2, K], [0, d1, d2, K]):
            parts, counts = [], np.zeros(N, np.uint32)
            for a, b in zip(cuts[:-1], cuts[1:]):
                segs, count = call(e, brk[a:b], p, rows=(a, b))
                parts.append(segs)
                counts += count
            allsegs = np.concatenate(parts)
            order = np.lexsort((allsegs[:, 1], allsegs[:, 0]))
            assert np.array_equal(allsegs[order], want) and np.array_equal(counts, wcount), cuts
        for a, b in ((20, 100), (60, 61), (119, K), (3, 3)):
            got = check(e, G, brk[a:b], p, rows=(a, b), what=(a, b))
            assert np.all(got[:, 1] >= a) and np.all(got[:, 2] < b)


def test_storages_and_precisions_agree():
    K, N = 260, 1025
    G = make(K, N, 0.05, 0.02, seed=900)
    brk = breaks(K, dom=[100])
    p = P(W=12, H=1, M=1, num=1, den=4, min_snp=15)
    want, wcount = model(G, brk, p)
    assert len(want) > 0
    for store, prec in (("int8", _lib.PREC_I8_EXACT), ("2bit", _lib.PREC_I8_EXACT), ("int8", _lib.PREC_F32_MFMA)):
        with gpca.GpcaEngine(precision=prec, storage=STORES[store]) as e:
            load(e, G)
            segs, count = call(e, brk, p)
            assert np.array_equal(segs, want) and np.array_equal(count, wcount), (store, prec)


def test_the_sample_mask_is_ignored_and_no_fitted_result_is_touched():
    G = make(300, 200, 0.1, 0.0, seed=950)
    brk = breaks(300)
    p = P(W=5, H=0, M=0, num=1, den=1, min_snp=5)
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        e.upload_genotypes_i8(G)
        e.snp_stats(gpca.QcConfig.none())
        K = int(e._lib.gpca_num_pca_snps(e._h))
        assert K == 300
        mask = np.zeros(200, np.uint8); mask[::2] = 1
        e.set_sample_mask(mask)
        e.rsvd(4, 4, 1, seed=3)
        sc, ev = e.scores(f64=True).copy(), e.eigenvalues().copy()
        want = check(e, G, brk, p)
        assert len(want) > 0 and np.any(want[:, 0] % 2 == 1)
        assert np.array_equal(e.scores(f64=True), sc) and np.array_equal(e.eigenvalues(), ev)


def test_refusals():
    N, K = 130, 60
    G = make(K, N, 0.1, 0.02, seed=1000)
    brk = breaks(K, dom=[30])
    p = P(W=5, H=1, M=1, num=1, den=2, min_snp=3)
    lib = _lib.load()
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        with pytest.raises(GpcaError) as ei:                                             # no genotypes
            call(e, brk[:0], p, rows=(0, 0))
        assert ei.value.status == _lib.GPCA_ERR_STATE and "gpca_roh" in str(ei.value)
        e.upload_genotypes_i8(G)
        with pytest.raises(GpcaError) as ei:                                             # no standardisation
            call(e, brk[:0], p, rows=(0, 0))
        assert ei.value.status == _lib.GPCA_ERR_STATE and "standardisation" in str(ei.value)
        load(e, G)
        check(e, G, brk, p)

        def raw(r0, r1, b, par, count, segs, cap, found=True):
            fv = ctypes.c_int64(0)
            rc = lib.gpca_roh(e._h, r0, r1, vp(b), None if par is None else ctypes.byref(par), vp(count), vp(segs), cap,
                              ctypes.byref(fv) if found else None)
            return rc, lib.gpca_last_error(e._h).decode()
        good = _lib.gpca_roh_params(5, 1, 1, 1, 2, 3, -1)
        count, segs = np.zeros(N, np.uint32), np.zeros((8, 5), np.uint32)
        assert raw(0, K, brk, good, count, segs, 8)[0] == _lib.GPCA_OK

        def with_(**kw):
            vals = dict(window_snp=5, window_het=1, window_missing=1, thr_num=1, thr_den=2, min_snp=3, max_het=-1)
            vals.update(kw)
            return _lib.gpca_roh_params(**vals)
        for par, word in ((with_(window_snp=0), "window_snp"), (with_(window_snp=65), "window_snp"), (with_(window_het=6), "window_het"),
                          (with_(window_het=-1), "window_het"), (with_(window_missing=6), "window_missing"), (with_(thr_num=3), "thr_num"),
                          (with_(thr_num=-1), "thr_num"), (with_(thr_den=0), "thr_den"), (with_(thr_den=(1 << 20) + 1, thr_num=1), "thr_den"),
                          (with_(min_snp=0), "min_snp"), (with_(max_het=-2), "max_het")):
            got = raw(0, K, brk, par, count, segs, 8)
            assert got[0] == _lib.GPCA_ERR_BAD_ARG and word in got[1] and "gpca_roh" in got[1], got
        for bad_byte in (1, 4, 5, 7, 128, 255):
            b = brk.copy(); b[17] = bad_byte
            got = raw(0, K, b, good, count, segs, 8)
            assert got[0] == _lib.GPCA_ERR_BAD_ARG and "brk[17]" in got[1], got
        b = brk.copy(); b[0] = 1                                                         # row row0 is taken as 3 whatever it holds
        assert raw(0, K, b, good, count, segs, 8)[0] == _lib.GPCA_OK
        for got, word in ((raw(0, K, None, good, count, segs, 8), "brk"), (raw(0, K, brk, None, count, segs, 8), "params"),
                          (raw(0, K, brk, good, None, segs, 8), "seg_count"), (raw(0, K, brk, good, count, segs, 8, found=False), "n_found"),
                          (raw(0, K, brk, good, count, None, 8), "segs"), (raw(0, K, brk, good, count, segs, 0), "segs"),
                          (raw(0, K, brk, good, count, segs, -1), "cap"), (raw(-1, K, brk, good, count, segs, 8), "rows"),
                          (raw(3, 2, brk, good, count, segs, 8), "rows"), (raw(0, K + 1, brk, good, count, segs, 8), "rows")):
            assert got[0] == _lib.GPCA_ERR_BAD_ARG and word in got[1] and "gpca_roh" in got[1], got
        with pytest.raises(GpcaError) as ei:                                             # num > den through the wrapper
            e.roh(brk, window_snp=5, window_threshold=(3, 2), min_snp=3)
        assert ei.value.status == _lib.GPCA_ERR_BAD_ARG
        with pytest.raises(ValueError):                                                  # a denominator above 2^20
            e.roh(brk, window_snp=5, window_threshold=0.0000001, min_snp=3)
        count[:] = 7
        assert raw(5, 5, brk[:0], good, count, None, 0)[0] == _lib.GPCA_OK and not count.any()   # an empty band writes zeros
        # a value outside the codes below N names its row, wherever the row lies: in a domain with windows, in one shorter than W
        for row, b in ((17, brk), (1, breaks(K, dom=[3]))):
            for bad in (3, -128, -126, 4, 64):
                Gb = G.copy(); Gb[row, N - 1] = bad
                load(e, Gb)
                with pytest.raises(GpcaError) as ei:
                    call(e, b, p)
                assert ei.value.status == _lib.GPCA_ERR_INVALID_GENOTYPE and f"row {row}" in str(ei.value), (row, bad)
                check(e, Gb, b[row + 1:], p, rows=(row + 1, K))                          # a band that does not hold the row is served
        e.set_standardization(np.ones(K, np.float32), np.ones(K, np.float32), np.zeros(K, np.uint8))
        with pytest.raises(GpcaError) as ei:                                             # K = 0: an empty keep mask
            call(e, brk[:0], p, rows=(0, 0))
        assert ei.value.status == _lib.GPCA_ERR_STATE and "no kept row" in str(ei.value)
    with gpca.GpcaEngine() as e:                                                         # a streamed handle
        e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), K, N, panel_rows=256, ring_slots=2, fused=False)
        e.snp_stats(gpca.QcConfig.none())
        with pytest.raises(GpcaError) as ei:
            call(e, brk, p)
        assert ei.value.status == _lib.GPCA_ERR_STATE and "panel" in str(ei.value)
    with gpca.GpcaEngine() as e:                                                         # a hooked (row-sharded) handle
        e.upload_genotypes_i8(G[:20].copy())
        e.set_allreduce_hook(lambda buf: None, 2, 0, 0)
        e.set_standardization(np.ones(20, np.float32), np.ones(20, np.float32), np.ones(20, np.uint8))
        with pytest.raises(GpcaError) as ei:
            call(e, brk[:20], p)
        assert ei.value.status == _lib.GPCA_ERR_STATE and "shard" in str(ei.value)


def test_the_timing_records():
    G = make(64, 300, 0.1, 0.02, seed=1100)
    with gpca.GpcaEngine(storage=_lib.STORE_INT8) as e:
        load(e, G)
        e.enable_timings(True)
        e.reset_timings()
        segs, _ = call(e, breaks(64), P(W=4, H=1, M=1, num=1, den=2, min_snp=2))
        recs = e.timings()
        assert len(segs) > 0 and "roh" in recs and recs["roh"]["launches"] == 1
