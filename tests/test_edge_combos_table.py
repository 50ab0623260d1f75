"""The case tables of tests/_combos.py, on the CPU: coverage, determinism, size, the builders' promises, and teeth.

Coverage: every pair of values of every two axes occurs in some case of each table; the pairs of EXEMPT occur too, but their band is
the nearest legal one, and EXEMPT names only pairs with one kept row or at most two samples.  Size: the caps of 48 and 56 cases keep
anybody from covering by enumeration (the products hold 10 800 and 3 024 cases).

Teeth, on each feature's own numpy model alone (no device): a case is worth running only if a kernel that read the wrong rows would give
other numbers.  So for every case of every feature
* band != full and K > 1: the expected output differs from that of the same-length band one row (sample) later and one earlier,
  wherever those exist (sample bands: compared on the same rows of the full symmetric matrix, so that the shapes agree);
* keep != all: it differs from the model of the same band indices with every row kept.  One exception, by construction: ``last`` on a
  row band keeps the first K rows, so the kept-row list IS the identity and the two models are equal (but for ld_score, whose windows
  are clipped at the last kept row); what the pattern holds against is a kernel that runs to M instead of K, so there the test asserts
  that the dropped rows hold calls;
* miss != none: it differs from the model with every missing call set to 0.
A feature may declare a case toothless for a reason that no data can change (``toothless``: f2 of one sample, an LD score of one row,
a ROH band shorter than its window); the expected output is then asserted to be all zero, which the device is still held to.  A case
that merely drew unlucky data names another seed in _combos.RESEED."""
import numpy as np
import pytest

import _combos as C


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f") for x, y in zip(a, b))


@pytest.mark.parametrize("kind,axes,cap", [("row", C.ROW_AXES, 48), ("sample", C.SAMPLE_AXES, 56)])
def test_coverage_determinism_and_size(kind, axes, cap):
    table = C.TABLES[kind]
    names = [n for n, _ in axes]
    every = {((a, u), (b, v)) for i, (a, va) in enumerate(axes) for b, vb in axes[i + 1:] for u in va for v in vb}
    assert C.pairs_of(table, axes) == every                                   # (the EXEMPT pairs too: their cases stay in the table)
    assert all(list(c) == names and all(c[n] in dict(axes)[n] for n in names) for c in table)
    seed = {"row": 1, "sample": 2}[kind]
    assert C.pairwise(axes, seed) == table and C.pairwise(axes, seed) == C.pairwise(axes, seed)
    assert len(table) <= cap, len(table)
    print(f"{kind}-band table: {len(table)} cases")
    for pair in C.EXEMPT[kind]:
        assert pair in every and any(p in ((("K", "1")), ("K", 1), ("N", 1), ("N", 2)) for p in pair), pair


def test_keep_patterns():
    for K in (1, 2, 31, 32, 33, 63, 64, 65, 127, 129, 255, 257, 513, 4097):
        for pat in C.KEEPS:
            M, keep = C.keep_for(K, pat)
            kr = np.flatnonzero(keep)
            assert keep.dtype == np.uint8 and keep.shape == (M,) and kr.size == K, (K, pat)
            if pat == "all":
                assert M == K
            if pat == "holes" and K > 2:
                assert not np.array_equal(kr, np.arange(K)) and len(set(np.diff(kr))) > 1 and M <= 3 * ((K + 1) // 2)
                assert all(keep[t:t + 3].sum() == 2 for t in range(0, M - 2, 3))
            if pat == "first":
                assert not keep[:32].any() and keep[32:].all()
            if pat == "last":
                assert M % 32 and not keep[(M - 1) // 32 * 32:].any() and keep[:K].all()


@pytest.mark.parametrize("kind", ["row", "sample"])
def test_bands_hold_their_class(kind):
    tile = 32 if kind == "row" else 128
    for c in C.TABLES[kind]:
        for R in (64, 128, 256) if kind == "row" else (None,):
            extent = C.k_of(c, R) if kind == "row" else c["N"]
            cls = c["band"]
            r0, r1 = C.band_for(extent, cls, tile)
            assert 0 <= r0 < r1 <= extent
            if any((("K" if kind == "row" else "N", c["K" if kind == "row" else "N"]), ("band", cls)) == p for p in C.EXEMPT[kind]):
                continue                                                       # the nearest legal band
            inside = [v for v in (r0, r1) if v not in (0, extent)] if cls != "lastrow" else []
            assert all(v % tile for v in inside) or extent <= 2, (extent, cls, r0, r1)
            want = {"full": (r0, r1) == (0, extent), "head": r0 == 0 and r1 < extent, "tail": r0 > 0 and r1 == extent,
                    "inner": 0 < r0 and r1 < extent and r1 - r0 > 1, "one": r1 == r0 + 1 and r0 > 0, "lastrow": (r0, r1) == (extent - 1, extent)}
            assert want[cls], (extent, cls, r0, r1)
            if cls == "inner" and extent > 2 * tile:
                assert r0 // tile != (r1 - 1) // tile, (extent, r0, r1)
            if kind == "row" and extent == 2 * R + 1 and cls in ("head", "tail", "inner"):
                assert r1 - r0 > R                                             # more than one workgroup's rows, and row0 > 0 in two of them


def test_missing_classes():
    M, keep = C.keep_for(33, "holes")
    G = np.ones((M, 17), np.int8)
    kr = np.flatnonzero(keep)
    assert np.array_equal(C.missing_for(G, "none", keep), G)
    two = C.missing_for(G, "2 %", keep) == C.MISSING
    assert 0 < two.sum() < 0.1 * G.size
    sp = C.missing_for(G, "special", keep) == C.MISSING
    assert sp[:, 17 // 3].all() and sp[kr[16]].all() and sp.sum() == M + 17 - 1


def _cases(feature):
    return [pytest.param(i, id=f"{i}-{C.case_id(c)}") for i, c in enumerate(C.table_of(feature))]


def _teeth(feature, i):
    f = C.FEATURES[feature]
    inp = C.build(feature, i)
    c, G, keep, band, K = inp["case"], inp["G"], inp["keep"], inp["band"], inp["K"]
    assert int(keep.sum()) == K and G.shape == (inp["M"], inp["N"]) and G.dtype == np.int8
    assert (c["miss"] == "none") == (not (G == C.MISSING).any())
    base = f.expect(inp, G, keep, band)
    why = f.toothless(inp)
    if why:
        assert all(not np.any(np.nan_to_num(x)) for x in base), (C.label(inp), why)
        return
    extent = K if f.table == "row" else inp["N"]
    if c["band"] != "full" and K > 1:
        for d in (1, -1):
            if 0 <= band[0] + d and band[1] + d <= extent:
                assert not _same(base, f.expect(inp, G, keep, (band[0] + d, band[1] + d))), (C.label(inp), "band shifted by", d)
    if c["keep"] != "all":
        if _same(base, f.expect(inp, G, None, band)):                             # the identity list: what bites is M > K
            assert c["keep"] == "last" and f.table == "row" and np.any(G[K:] > 0), (C.label(inp), "every row kept")
    if c["miss"] != "none":
        assert not _same(base, f.expect(inp, np.where(G == C.MISSING, 0, G).astype(np.int8), keep, band)), (C.label(inp), "missing as 0")


@pytest.mark.parametrize("i", _cases("group_counts"))
def test_teeth_group_counts(i):
    _teeth("group_counts", i)


@pytest.mark.parametrize("i", _cases("f2_blocks"))
def test_teeth_f2_blocks(i):
    _teeth("f2_blocks", i)


@pytest.mark.parametrize("i", _cases("sample_counts"))
def test_teeth_sample_counts(i):
    _teeth("sample_counts", i)


@pytest.mark.parametrize("i", _cases("roh"))
def test_teeth_roh(i):
    _teeth("roh", i)


@pytest.mark.parametrize("i", _cases("ld_score"))
def test_teeth_ld_score(i):
    _teeth("ld_score", i)


@pytest.mark.parametrize("i", _cases("king"))
def test_teeth_king(i):
    _teeth("king", i)


@pytest.mark.parametrize("i", _cases("grm"))
def test_teeth_grm(i):
    """... and every case lies in the exact regime of test_gpu_grm_exact.py (big < 2^53) under both scalings"""
    _teeth("grm", i)
    f = C.FEATURES["grm"]
    inp = C.build("grm", i)
    for scaling in f.SCALINGS:
        assert f.model(inp, inp["G"], inp["keep"], scaling).big < 2 ** 53, (C.label(inp), scaling)


def test_reseed_names_cases_of_the_tables():
    for (feature, i), seed in C.RESEED.items():
        assert 0 <= i < len(C.table_of(feature)) and seed > 0
