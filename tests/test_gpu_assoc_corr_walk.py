"""The item walk of k_assoc_spa and k_assoc_firth (assoc_spa.hip, assoc_firth.hip, assoc_stage.h) at its edges, crossed: a workgroup's
second and later items (GPCA_ASP_SLOTS = 1, 2, 3), the staging chunks two to five, the kept-row map under a keep mask with holes and
under one kept row, fewer than 1024 slots (N = 32769), bands that start past kept row 0, 2-bit rows and an f32-MFMA handle, and the
second list range under the saddle-point correction.  The cases are those of tests/_corr_walk.py (a pairwise table and the hand-written
cases beside it; tests/test_assoc_corr_walk_table.py holds the table to its promises on the CPU).

Nothing here has a tolerance of its own.  Every case asserts
 (a) bits: the full call under the case's forced slot count equals the full call with the hook unset (np.array_equal, NaN-aware, every
     output key), and the case bites: with s forced workgroups at least 2 s + 1 items are corrected; the case's band equals the same
     rows of the full call; a 2-bit or f32-MFMA handle equals int8; stats, ua and rowinfo equal gpca_assoc_logistic_score's;
 (b) model: the hook-unset int8 result is held on the kept rows to the numpy restatement by the check_against_restatement of
     test_gpu_assoc_spa.py / test_gpu_assoc_firth.py (spa_bars / firth_bars with their dg term), the genotypes indexed through the
     keep mask.  The saddle-point check may skip an item only where near_decision says so, at most 2 % of a case's items; Firth's
     skips none;
 (c) the model can tell (test_model_can_tell_*, on the device's own output): at N = 16385 the restatement with the samples from 8192 on
     set to 0 breaks the check for every corrected item, and under a keep mask with holes the restatement fed row row0 + i of the
     unmasked matrix breaks it for the corrected items whose kept row differs from its index.
test_spa_across_the_list_range is the twin of test_gpu_assoc_firth.test_across_the_list_range with every ninth row dropped, 2-bit rows
and a forced slot count.

Records (one MI355X; records, not thresholds).  46 walk cases (33 of the pairwise table, 13 hand-written; 11 forced counts dropped, named
in the case ids), 4 tell cases and the list range: 51 tests, 11.5 s of wall time for the module; the slowest case takes 1.14 s
(45-firth-dense-N32769-21x0-slots2-all-inner-f32; the four slowest are the N = 32769 ones, 0.8 to 1.1 s, most of it the host's null
fits and the numpy model), the list range 0.76 s, against 0.66 s for the slowest test of test_gpu_assoc_firth.py in the same run.  The
walk cases hold 6 063 items to the model, 2 151 of them corrected, none skipped, no status 2.  Worst fraction of a bar: saddle point,
zeta 4.0e-6, -log10 p 1.3e-5; Firth, beta 2.2e-5, -log10 p 0.010, se 2.3e-3, D 0.031, at most 13 passes.  The list range corrects 2 618
of 1 052 432 items, 2 610 in the first range and 8 in the second; 23 rows around the boundary and at the end (25 corrected items) are held
to the model (zeta 3.1e-6, -log10 p 2.0e-6).  The tell cases: 7 and 12 corrected items leave their bar without the later chunks, 31 of 31
and 50 of 50 when fed the unmasked row.  Two figures of the issue are off by a little and are stated here as the code has them:
asp_slots(32769) is 1022 (a slice of 32 832 doubles), and 74 000 rows with every ninth dropped keep 65 777 rows (1 052 432 items)."""
import os

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib

import _corr_walk as W
import test_gpu_assoc_firth as tf
import test_gpu_assoc_spa as ts
from test_gpu_assoc_score import VIF, load, same

pytestmark = pytest.mark.gpu

ENGINES = {"int8": dict(storage=_lib.STORE_INT8), "2bit": dict(storage=_lib.STORE_2BIT),
           "f32": dict(storage=_lib.STORE_INT8, precision=_lib.PREC_F32_MFMA)}
IDS = [W.case_id(i) for i in range(len(W.CASES))]
MOD = {"spa": ts, "firth": tf}
STATUS = {"spa": "spa_status", "firth": "firth_status"}


@pytest.fixture
def slots_env():
    old = os.environ.get("GPCA_ASP_SLOTS")

    def set_slots(s):
        if s is None:
            os.environ.pop("GPCA_ASP_SLOTS", None)
        else:
            os.environ["GPCA_ASP_SLOTS"] = str(s)         # (the library reads it per call)
    yield set_slots
    set_slots(old)


def call(e, inp, rows=None):
    kw = dict(include=inp["inc"], max_vif=VIF, rows=rows, ua=True)
    if inp["corr"] == "spa":
        return e.assoc_logistic_spa(inp["Y"], inp["C"], spa_z=inp["cutoff"], **kw)
    return e.assoc_logistic_firth(inp["Y"], inp["C"], firth_z=inp["cutoff"], **kw)


def take(r, idx):
    """the rows idx of a result"""
    return {k: v[idx] for k, v in r.items()}


def model(inp, r, Gk, rows=None):
    """check_against_restatement of the correction's own module over the rows `rows` of r (all of them by default); Gk: the genotypes of
    r's rows.  Returns (items, skipped, the worst fraction of each bar seen)."""
    m = MOD[inp["corr"]]
    idx = np.arange(r["z"].shape[0]) if rows is None else np.asarray(rows, np.int64)
    before = dict(m.WORST)
    for k in m.WORST:
        m.WORST[k] = 0
    try:
        items, other = m.check_against_restatement(take(r, idx), Gk[idx], inp["inc"], inp["nulls"], inp["cutoff"], inp["Pc"])
    finally:
        seen = dict(m.WORST)
        for k in m.WORST:                                 # (the modules print their worst "so far": it stays a running maximum)
            m.WORST[k] = max(before[k], seen[k])
    return items, (other if inp["corr"] == "spa" else 0), seen


def run_case(inp, slots_env):
    """(a) of the module docstring; returns the hook-unset int8 result of the full call"""
    s, (a, b) = inp["slots"], inp["band"]
    slots_env(None)
    with gpca.GpcaEngine(**ENGINES["int8"]) as e:
        load(e, inp["G"], inp["keep"])
        r = call(e, inp)
        score = e.assoc_logistic_score(inp["Y"], inp["C"], include=inp["inc"], max_vif=VIF, ua=True)
        if s is not None:
            slots_env(s)
            forced = call(e, inp)
    for k, v in score.items():                            # pass-through: the score call's bits
        assert same(v, r[k]), k
    st = r[STATUS[inp["corr"]]]
    assert r["z"].shape == (inp["K"], inp["T"]) and np.all((st == 0) | (st == 1))
    assert np.array_equal(st == 1, W.listed(inp, r))      # what the flag kernel listed was corrected, and nothing else
    if s is not None:
        assert int((st == 1).sum()) >= 2 * s + 1, ("the case cannot bite", int((st == 1).sum()))
        for k, v in r.items():
            assert same(v, forced[k]), ("forced slots", s, k)
    if inp["eng"] != "int8" or a != 0 or b != inp["K"]:
        slots_env(s)
        with gpca.GpcaEngine(**ENGINES[inp["eng"]]) as e:     # the case's handle, band and slot count together
            load(e, inp["G"], inp["keep"])
            band = call(e, inp, rows=(a, b))
        for k, v in band.items():
            assert v.shape[0] == b - a and same(v, r[k][a:b]), (inp["eng"], (a, b), k)
    slots_env(None)
    return r


@pytest.mark.parametrize("i", range(len(W.CASES)), ids=IDS)
def test_walk_case(i, slots_env):
    inp = W.build(i)
    r = run_case(inp, slots_env)
    Gk = inp["G"][inp["kept"]]
    items, skipped, worst = model(inp, r, Gk)
    st = r[STATUS[inp["corr"]]]
    print(f"{IDS[i]}: K {inp['K']}, band {inp['band']}, slots {inp['slots']}: {int((st == 1).sum())} of {st.size} items corrected; model on "
          f"{items} items, skipped {skipped}; worst / bar: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert items == inp["K"] * inp["T"] and skipped <= 0.02 * items
    if inp["special"] and inp["case"]["keep"] != "one":   # the special rows are among the kept ones, wherever the mask put them
        k = {int(o): j for j, o in enumerate(inp["kept"])}
        assert r["flipped"][k[0]] == 1.0 and r["flipped"][k[3]] == 0.0
        assert np.all(np.isnan(r["log10p"][k[2]])) and np.all(np.isnan(r["log10p"][k[inp["L"] - 1]]))


def _each_corrected(inp, r, Gk):
    st = r[STATUS[inp["corr"]]]
    for i, t in zip(*np.nonzero(st == 1)):
        one = {k: (v[i:i + 1, t:t + 1] if v.ndim >= 2 else v[i:i + 1]) for k, v in r.items()}      # (per item [K][T]..., per row [K])
        yield int(i), int(t), one, Gk[i:i + 1], dict(inp, nulls=inp["nulls"][t:t + 1], T=1)


def _tell_case(corr, N, tp, keep):
    c = dict(corr=corr, cut="dense", N=N, tp=tp, slots=None, keep=keep, band="full", eng="int8")
    i = next((j for j, x in enumerate(W.CASES) if all(x[k] == v for k, v in c.items() if k not in ("slots", "band", "eng"))), None)
    assert i is not None, c
    return W.build(i)


@pytest.mark.parametrize("corr", ["spa", "firth"])
def test_model_can_tell_a_later_chunk(corr, slots_env):
    """N = 16385: with the samples from 8192 on set to 0 in the restatement's genotypes, every corrected item leaves its bar.  Rows 5, 6
    and 7 of Firth's inputs (two singletons and a dozen carriers, all among the first samples) hold no call but 0 past sample 8192: no
    restatement can tell for them, so this test's keep mask drops them from both corrections' inputs (asserted: every kept row that
    has a corrected item holds an observed non-zero call of an included sample past 8192)."""
    inp = _tell_case(corr, 16385, "2x3", "holes" if corr == "firth" else "all")
    inp["keep"] = np.ones(inp["L"], np.uint8)
    inp["keep"][[5, 6, 7]] = 0
    inp["kept"] = np.flatnonzero(inp["keep"])
    slots_env(None)
    with gpca.GpcaEngine(**ENGINES["int8"]) as e:
        load(e, inp["G"], inp["keep"])
        r = call(e, inp)
    Gk = inp["G"][inp["kept"]]
    cut = Gk.copy()
    cut[:, 8192:] = 0
    late = ((Gk[:, 8192:] > 0) & (inp["inc"][None, 8192:] == 1)).any(1)
    assert np.all(late[(r[STATUS[corr]] == 1).any(1)])
    seen = 0
    for i, t, one, g1, inp1 in _each_corrected(inp, r, Gk):
        assert model(inp1, one, g1)[1] == 0               # (the item itself passes, alone, as it does in its case)
        with pytest.raises(AssertionError):
            model(inp1, one, cut[i:i + 1])
        seen += 1
    print(f"{corr}: {seen} corrected items, each outside its bar without the chunks past the first")
    assert seen >= 5


@pytest.mark.parametrize("corr", ["spa", "firth"])
def test_model_can_tell_the_kept_row_map(corr, slots_env):
    """holes in the keep mask, N = 8257: fed row row0 + i of the unmasked matrix, the restatement breaks for the corrected items whose
    kept row differs from its index (all of them but the rows before the first hole)"""
    inp = _tell_case(corr, 8257, "2x3", "holes")
    slots_env(None)
    with gpca.GpcaEngine(**ENGINES["int8"]) as e:
        load(e, inp["G"], inp["keep"])
        r = call(e, inp)
    Gk, Gid = inp["G"][inp["kept"]], inp["G"][:inp["K"]]
    moved = inp["kept"] != np.arange(inp["K"])
    assert moved.any() and not moved.all()
    seen = broken = 0
    for i, t, one, g1, inp1 in _each_corrected(inp, r, Gk):
        if not moved[i] or np.array_equal(Gid[i], Gk[i]):
            continue
        seen += 1
        try:
            skipped = model(inp1, one, Gid[i:i + 1])[1]
        except AssertionError:
            broken += 1
        else:
            assert skipped == 0 or corr == "spa"
    print(f"{corr}: {broken} of {seen} corrected items on moved rows leave their bar when fed the unmasked row")
    assert seen >= 5 and broken == seen


def test_spa_across_the_list_range(slots_env):
    """N = 63, T = 16, Pc = 1, 2-bit rows, 74 000 rows with every ninth dropped (rows 0, 9, ...: 8 223 of them): 65 777 kept rows,
    1 052 432 items, the second list range starts at item 2^20 = kept row 65 536 (loaded row 73 729).  spa_z = 3; one call with the
    hook unset, one with GPCA_ASP_SLOTS = 3."""
    N, T, Pc, M = 63, 16, 1, 74000
    rng = np.random.default_rng(63016)
    p = rng.uniform(0.05, 0.5, M)[:, None]
    G = ((rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8))
    G[rng.random((M, N)) < 0.01] = -127
    Y = (rng.random((N, T)) < 0.3).astype(np.float64)
    Y[:3], Y[3:6] = 1.0, 0.0
    Cm = rng.standard_normal((N, Pc))
    inc = np.ones(N, np.uint8)
    keep = np.ones(M, np.uint8); keep[::9] = 0
    kept = np.flatnonzero(keep)
    K = kept.size
    assert K == 65777 and K * T == 1052432 > 2 ** 20 == 65536 * T and kept[65536] == 73729
    nulls = ts.rebuild(Y, Cm, inc)
    kw = dict(include=inc, max_vif=VIF, spa_z=3.0, ua=True)
    slots_env(None)
    with gpca.GpcaEngine(storage=_lib.STORE_2BIT) as e:
        load(e, G, keep)
        r = e.assoc_logistic_spa(Y, Cm, **kw)
        score = e.assoc_logistic_score(Y, Cm, include=inc, max_vif=VIF, ua=True)
        slots_env(3)
        forced = e.assoc_logistic_spa(Y, Cm, **kw)
        band = e.assoc_logistic_spa(Y, Cm, rows=(65000, 65700), **kw)
    slots_env(None)
    for k, v in score.items():
        assert same(v, r[k]), k
    for k, v in r.items():
        assert same(v, forced[k]), k
    for k, v in band.items():
        assert same(v, r[k][65000:65700]), k
    z, st = r["z"], r["spa_status"]
    flagged = np.isfinite(z) & (np.abs(z) >= 3.0) & (r["ua"][:, :, 0] != 0.0)
    assert np.all(st[flagged] >= 1) and np.all(st[~flagged] == 0)
    lo, hi = flagged[:65536], flagged[65536:]
    print(f"{int(flagged.sum())} of {flagged.size} items corrected: {int(lo.sum())} in the first range, {int(hi.sum())} in the second")
    assert lo.sum() > 100 and hi.sum() > 0 and flagged.sum() >= 7
    # the flagged items of the rows around the boundary and of the last rows, against the restatement
    rows = sorted(set(np.flatnonzero(flagged[65000:65700].any(1))[:40] + 65000) | set(np.flatnonzero(flagged[65536:].any(1))[:10] + 65536)
                  | set(np.flatnonzero(flagged[K - 200:].any(1))[-10:] + K - 200))
    inp = dict(corr="spa", inc=inc, nulls=nulls, cutoff=3.0, Pc=Pc)
    items, skipped, worst = model(inp, r, G[kept], rows)
    corrected = int((st[rows] == 1).sum())
    print(f"{len(rows)} rows, {items} items, {corrected} corrected, skipped {skipped}; worst / bar: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert corrected >= 10 and skipped <= 0.02 * items and any(i >= 65536 for i in rows)
