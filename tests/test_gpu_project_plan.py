"""gpca_project under forced launch plans: the steady-state trips of k_project's register ring (project.hip, prj_plan of plan_math.h).

THE GAP THIS CLOSES.  A wave of k_project walks its rows in trips of four 32-row blocks through a 4-stage register ring.  In every trip
but the last ``more = 1``: the buffer resources are re-based on gp + kb * 32 * ldr, the three prefetches of the next trip use the offsets
(4 more + i) L32, the row mask index is 4 more + i and the plane offsets are (4 more + i) TKB.  prj_plan gives a wave rows_per_wave rows;
with the tuned default of 2 048 waves a wave gets more than 128 rows only when Mpad (Npad / 64) > 262 144, which no gpca_project case of
the suite reaches -- every one of them runs one trip per wave with more = 0 -- while at 1M x 10k a wave runs about 650 trips.  The same
holds for GPCA_PROJECT_LAZY_B = 1 (LAZYB: the indicator planes are loaded behind the ballot and not carried in the ring).

THE PLANS (``prj_plan``: plan_math.h's restated; Mpad = round_up(M, 128), Npad = round_up(N, 256 | 1024), target = max(4, gtt_waves) or
2 048).  test_restated_plans_reach_the_trips_the_shapes_are_chosen_for (CPU) asserts what each case of PLANS reaches, trips per row chunk:
    int8 rows, N = 257 (Npad 512, 8 sample blocks)               2-bit rows, N = 1 025 (Npad 2 048, 32 sample blocks)
      M = 129, 256  gtt_waves = 4    W = 1: 2 trips                M = 129   gtt_waves = 4     W = 1: 2 trips
      M = 257       gtt_waves = 4    W = 1: 3 trips                M = 257   gtt_waves = 4     W = 1: 3 trips
      M = 4097      gtt_waves = 4    W = 1: 33 trips               M = 4097  gtt_waves = 4     W = 1: 33 trips
      M = 4097      gtt_waves = 16   W = 2: 17, 16 trips           M = 4097  gtt_waves = 64    W = 2: 17, 16 trips
      M = 4097      gtt_waves = 24   W = 3: 11, 11, 11 trips       M = 1601  gtt_waves = 128   W = 4: 4, 4, 4, 1 trips
      M = 1601      gtt_waves = 32   W = 4: 4, 4, 4, 1 trips
and, under the default plan (gtt_waves = 0), one trip in every chunk of every one of these shapes: that states the gap, and a planner
change that moves a shape off its trips turns the CPU test red.  The streamed case (M = 5 000, panels of 1 024 rows, gtt_waves = 4) runs
8 trips per panel and 40 resident.

WHAT IS ASSERTED ON THE DEVICE, per case (all three MODES of test_gpu_exact_pass.py, k = 33, ``make_inputs`` families pow2 and generic,
1 % missing calls):
  1. check_against_bars and used == model["used"] of test_gpu_exact_pass.py, unchanged;
  2. the scores and used under the forced plan are the bits of the same call under the default plan;
  3. GPCA_PROJECT_LAZY_B = 1 gives the bits of GPCA_PROJECT_LAZY_B = 0, under both plans;
  4. streamed panels give the resident bits under the forced plan, and both sit inside the bars.
2 and 3 are derived, not hoped for: everything that depends on the plan is a sum of exact integers -- the i32 accumulators of a wave
(|g| |digit| <= 128 per row, at most 4 224 rows), combine_digits in f64, and the f64 fold of the W partials in launch_accum_y_i8 -- and
test_integer_sums_stay_below_2_to_the_53 (CPU) asserts from the model that max |Yint_a|, |Yint_b| < 2^53 for every case.  c, the digit
scales and the finish do not see the plan.  No tolerance here is new.

Measured on one MI355X (records, not thresholds; each test prints its own with -s), the largest fraction of a bar over every case,
sample and column:  against the model 0.0078 (int8), 0.0153 (2-bit, 3 planes), 0.0153 (2-bit, 4 planes);  against ref_project 0.19 / 0.30 /
0.15.  Every bit-identity held.  The module's wall time there: 6 s for its 74 device cases (34 forced plans, the same 34 under
GPCA_PROJECT_LAZY_B = 1, 6 streamed); the 3 CPU cases take 4 s.
Two value-only defects compiled into k_project on scratch copies, each run once.  The ring's B2 prefetch reloading the planes of the
trip before ((4 more + 2) TKB -> 2 TKB; the default plan cannot see it: with more = 0 the two offsets are the same): all 34 forced-plan
cases and the 6 streamed ones went red, and so did 28 of the 34 LAZY_B comparisons (LAZYB loads the indicator planes at the block's own
offset, so the variants part wherever a block of that ring slot holds a missing call).  That copy also left sample t = 1 out of the
ballot, which the LAZY_B comparisons cannot see (both variants share the ballot).  The B1 prefetch taking the row mask of the trip before
left this module green -- every row of ``make_inputs`` is a model row -- and was caught by the rows outside the model of
tests/test_gpu_ballot_edges.py."""
import functools

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from test_gpu_exact_pass import MODES, check_against_bars, exact_pass_model, few_ties, make_inputs
from test_gpu_k2_pass import round_up, waves_target

K = 33
MISS = 0.01
FAMILIES = ["pow2", "generic"]
LAZY_ENV = "GPCA_PROJECT_LAZY_B"


# ---- prj_plan of plan_math.h, restated -------------------------------------------------------------------------------------------------------
def prj_plan(Mpad, Npad, target):
    nblocks = Npad // 64
    W = max(target // nblocks, 1, (Mpad + (1 << 22) - 1) >> 22)
    W = max(min(W, Mpad // 128), 1)
    rpw = round_up(-(-Mpad // W), 128)
    W = -(-Mpad // rpw)
    return dict(ngroups=(nblocks + 3) // 4, W=W, rows_per_wave=rpw, grid=(nblocks + 3) // 4 * W)


def chunk_trips(rows, N, packed, gtt_waves):
    """trips of the ring (128 rows each) in every row chunk of one launch over `rows` rows"""
    Mpad = round_up(rows, 128)
    p = prj_plan(Mpad, round_up(N, 1024 if packed else 256), waves_target(gtt_waves))
    ch = [min(Mpad, (w + 1) * p["rows_per_wave"]) - w * p["rows_per_wave"] for w in range(p["W"])]
    assert sum(ch) == Mpad and all(c > 0 and c % 128 == 0 for c in ch)
    return tuple(c // 128 for c in ch)


# (rows kind, M, N, gtt_waves) -> the trips per row chunk the shape was chosen for
PLANS = {("int8", 129, 257, 4): (2,), ("int8", 256, 257, 4): (2,), ("int8", 257, 257, 4): (3,), ("int8", 4097, 257, 4): (33,),
         ("int8", 4097, 257, 16): (17, 16), ("int8", 4097, 257, 24): (11, 11, 11), ("int8", 1601, 257, 32): (4, 4, 4, 1),
         ("2bit", 129, 1025, 4): (2,), ("2bit", 257, 1025, 4): (3,), ("2bit", 4097, 1025, 4): (33,), ("2bit", 4097, 1025, 64): (17, 16),
         ("2bit", 1601, 1025, 128): (4, 4, 4, 1)}
ROW_MODES = {"int8": ["int8"], "2bit": ["2bit", "2bit4"]}
CASES = [(mode, M, N, w) for (rows, M, N, w) in PLANS for mode in ROW_MODES[rows]]
STREAM = dict(M=5000, N=257, panel_rows=1024, gtt_waves=4)


def test_restated_plans_reach_the_trips_the_shapes_are_chosen_for():
    for (rows, M, N, w), trips in PLANS.items():
        assert chunk_trips(M, N, rows == "2bit", w) == trips, (rows, M, N, w)
        # the default plan: every chunk of every one of these shapes is ONE trip (more = 0 only) -- the gap this module closes
        assert set(chunk_trips(M, N, rows == "2bit", 0)) == {1}, (rows, M, N)
    for rows in ("int8", "2bit"):
        got = [t for key, t in PLANS.items() if key[0] == rows]
        assert any(len(t) == 1 and t[0] >= 2 for t in got)                          # W = 1 with at least 2 trips
        assert (2,) in got and (3,) in got                                          # more = 1 then 0; more = 1, 1, then 0
        assert any(len(t) >= 2 and min(t) >= 2 for t in got)                        # W >= 2, every chunk multi-trip
        assert any(len(t) >= 2 and max(t) >= 2 and t[-1] == 1 for t in got)         # a multi-trip plan whose last chunk is one trip
    # the streamed case: every panel (the last holds 904 rows, padded to 1 024) runs 8 trips, the resident matrix 40; by default one each
    M, N, pr, w = STREAM["M"], STREAM["N"], STREAM["panel_rows"], STREAM["gtt_waves"]
    for packed in (False, True):
        for r0 in range(0, M, pr):
            assert chunk_trips(min(pr, M - r0), N, packed, w) == (8,)
            assert set(chunk_trips(min(pr, M - r0), N, packed, 0)) == {1}
        assert chunk_trips(M, N, packed, w) == (40,) and set(chunk_trips(M, N, packed, 0)) == {1}


@functools.lru_cache(maxsize=None)
def inputs(M, N, family):
    """(G, mu, sigma, W) of one shape and family: computed once, shared, never modified"""
    out = make_inputs(M, N, K, MISS, family, seed=1000 * N + M)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("family", FAMILIES)
def test_integer_sums_stay_below_2_to_the_53(family):
    """what makes the bit-identity of two plans a derived fact: every integer the plan can regroup is exact in f64"""
    shapes = sorted({(M, N) for (_, M, N, _) in PLANS} | {(STREAM["M"], STREAM["N"])})
    for M, N in shapes:
        for nd in (3, 4):
            m = exact_pass_model(*inputs(M, N, family), nd)
            top = max(float(np.max(np.abs(m["Yia"]))), float(np.max(np.abs(m["Yib"]))))
            print(f"M={M} N={N} nd={nd} {family}: max |Yint| = 2^{np.log2(max(top, 1)):.1f}")
            assert top < 2.0 ** 53 and m["digits_ok"] and few_ties(m)
            assert 128 * 128 * round_up(M, 128) < 2 ** 31                           # one wave's i32 accumulator over ALL the rows


# ---- the device ------------------------------------------------------------------------------------------------------------------------------
_DEV = {}
RECORD = {}


def project_once(monkeypatch, mode, M, N, family, gtt_waves, lazy):
    """(scores, used) of one call; cached per (mode, shape, family, plan, LAZYB)"""
    key = (mode, M, N, family, gtt_waves, lazy)
    if key not in _DEV:
        store, planes, _ = MODES[mode]
        G, mu, sigma, W = inputs(M, N, family)
        monkeypatch.setenv(LAZY_ENV, str(lazy))
        with gpca.GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=store, digit_planes=planes, gtt_waves=gtt_waves) as e:
            e.upload_genotypes_i8(G)
            _DEV[key] = e.project(mu, sigma, W)
    return _DEV[key]


def record(mode, fm, ft):
    a, b = RECORD.get(mode, (0.0, 0.0))
    RECORD[mode] = (max(a, fm), max(b, ft))
    print("largest fractions of the bars so far (model, ref_project):", RECORD)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("mode,M,N,gtt_waves", CASES)
def test_project_forced_plan(monkeypatch, mode, M, N, gtt_waves, family):
    nd = MODES[mode][2]
    G, mu, sigma, W = inputs(M, N, family)
    what = f"project {mode} M={M} N={N} gtt_waves={gtt_waves} {family}"
    sc, used = project_once(monkeypatch, mode, M, N, family, gtt_waves, 0)
    m, fm, ft = check_against_bars(sc, G, mu, sigma, W, nd, family == "generic", what)
    record(mode, fm, ft)
    assert np.array_equal(used, m["used"]), what
    assert np.all(sc[:, K // 2] == 0.0) and np.all(sc[N // 2] == 0.0) and used[N // 2] == 0, what
    sc0, used0 = project_once(monkeypatch, mode, M, N, family, 0, 0)
    assert np.array_equal(sc, sc0) and np.array_equal(used, used0), what + ": the forced plan moved a bit of the default plan's result"


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("mode,M,N,gtt_waves", CASES)
def test_project_forced_plan_lazy_b(monkeypatch, mode, M, N, gtt_waves, family):
    """LAZYB = true: the indicator planes loaded behind the ballot, at the offsets of the trip -- the bits of LAZYB = false"""
    what = f"project {mode} M={M} N={N} gtt_waves={gtt_waves} {family}"
    for w in (gtt_waves, 0):
        sc, used = project_once(monkeypatch, mode, M, N, family, w, 0)
        scl, usedl = project_once(monkeypatch, mode, M, N, family, w, 1)
        assert np.array_equal(scl, sc) and np.array_equal(usedl, used), what + f": {LAZY_ENV}=1 moved a bit (gtt_waves={w})"


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("mode", list(MODES))
def test_project_streamed_panels_forced_plan(monkeypatch, mode, family):
    """8 trips per panel of 1 024 rows against 40 resident: the same bits, inside the bars, with either LAZYB"""
    store, planes, nd = MODES[mode]
    M, N, w = STREAM["M"], STREAM["N"], STREAM["gtt_waves"]
    G, mu, sigma, W = inputs(M, N, family)
    what = f"project streamed {mode} M={M} N={N} gtt_waves={w} {family}"
    sc, used = project_once(monkeypatch, mode, M, N, family, w, 0)
    m, fm, ft = check_against_bars(sc, G, mu, sigma, W, nd, family == "generic", what + " (resident)")
    record(mode, fm, ft)
    assert np.array_equal(used, m["used"]), what
    for lazy in (0, 1):
        monkeypatch.setenv(LAZY_ENV, str(lazy))
        with gpca.GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=store, digit_planes=planes, gtt_waves=w) as e:
            e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), M, N, panel_rows=STREAM["panel_rows"], ring_slots=2,
                          fused=False)
            scs, useds = e.project(mu, sigma, W)
        check_against_bars(scs, G, mu, sigma, W, nd, family == "generic", what + f" (streamed, {LAZY_ENV}={lazy})")
        assert np.array_equal(scs, sc) and np.array_equal(useds, used), what + f": streamed != resident ({LAZY_ENV}={lazy})"
    sc0, used0 = project_once(monkeypatch, mode, M, N, family, 0, 0)
    assert np.array_equal(sc, sc0) and np.array_equal(used, used0), what
