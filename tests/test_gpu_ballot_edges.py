"""One missing call at a time: the wave-uniform ballots of k_king, k_project and k_pcrelate (king.hip, project.hip, pcrelate.hip).

THE GAP THIS CLOSES.  Three kernels skip their missing-call MFMAs on a wave-uniform ballot: k_king per 32-row block (H M^T, M H^T, M M^T),
k_project per 32-row block (the indicator planes and the per-sample count) and the den pass of k_pcrelate per 16-row stage (the i32
product of the invalid indicators, run only when both sides of the wave hold one).  At the suite's missing rates, 0 and at least 1 %,
every block of a call is loud or every block is quiet, so the ballot decides nothing a test can see: a side or a sub-tile left out of the
vote, the kept-row mask applied to the wrong half, a count gated on the wrong flag would all pass.  Here ONE call (for the pair products:
two calls of one row) is missing in an otherwise complete matrix, so exactly the waves that hold it must take the missing path, every
other wave must skip it, and the result must be the model's either way.

THE PLACEMENTS (``lonely``: the row keeps heterozygous and homozygous partners).  Both storages everywhere.
  gpca_king      M = 200 (four 64-row stages, both LDS buffers), N = 257 (three tile rows: diagonal and off-diagonal tiles).  Rows {0, 15,
                 16, 31, 32, 63, 64, M - 1} x samples {0, 31, 32, 63, 64, 95, 96, 127, 128, N - 1}: every wa, both column halves of a
                 wave, both j sub-tiles, the a side and the b side.  Pairs of missing calls in one row (the only way M M^T shows below
                 the diagonal) at rows {16, M - 1}.  Keep masks: the lonely row the only kept row; a kept row alone in its 32-row block;
                 a row that is not kept (the clean matrix's bits).  M = 4 097 with the call in the last block.  Model: ref_king of
                 test_gpu_king.py, counts and kinship compared with np.array_equal.
  gpca_project   M = 257 under gtt_waves = 4 (3 trips of the register ring, test_gpu_project_plan.py) and M = 129 under the default plan
                 (two one-trip chunks), N = 257, k = 33 (the count is taken in the first column half only, the correction in both).
                 Rows {0, 15, 16, 31, 32, 64, 96, 127, 128, 160, M - 1} below M (each ring slot, both lane halves, the trip boundary) x
                 samples {0, 1, 62, 63, 64, N - 1} (both t, the wave boundary, the second workgroup); GPCA_PROJECT_LAZY_B 0 and 1, bit
                 for bit.  A lonely call in a row outside the model (rows 32, 128, 160, 192, 224: a first-trip block and every slot of
                 the ring in a later trip, whose row mask the prefetch fetches): the clean matrix's bits, used unchanged.  Model and bars:
                 exact_pass_model / check_against_bars of test_gpu_exact_pass.py, unchanged.
  gpca_pcrelate  P = 0, tau = 0.05, row frequencies in [0.2, 0.8], no all-missing sample or row: validity is observedness, asserted from
                 the device's mu bits with valid_f32 before anything is compared.  330 rows of which K = 300 are kept, N = 257.  Kept
                 rows {0, 7, 8, 15, 16, 255, 256, K - 1} x sample pairs (100, 5) (a and b side of one wave), (40, 10) (both inside one
                 wave's b side, one in its a side), (130, 140) (a side only in tile (1, 0)), (5, 10) (b side only there), (32, 31),
                 (64, 63), (128, 127), (256, 0).  nsnp exactly ref_pairs'; the kinship inside test_gpu_pcrelate.py's bar.

TEETH (CPU, unmarked).  Mutants of the models must move a bit on the lonely cases they can touch and leave the clean matrix alone:
ref_king with H M^T, M H^T or M M^T dropped, or with a missing call on a row that is not kept counted (``king_sums``, which restates
ref_king and is asserted equal to it); exact_pass_model with the lonely call's b o W correction dropped (it must break the bar against
the model at EVERY placement of both shapes and both plane counts: a lonely correction is about mu r |W| and the f32 term of the bar
grows with M) or its count dropped; ref_pairs with the product of the invalid indicators dropped.

No tolerance here is new: every comparison is exact equality or a bar that an earlier module derived.

Measured on one MI355X (records, not thresholds; each test prints its own with -s).  gpca_king and the pair count: exact.  gpca_project,
the largest fraction of the bar against the model over the lonely cases: 0.0044 at M = 257, 0.0069 at M = 129 (both storages); on the
CPU a dropped lonely correction is at least 297 (M = 257) and 676 (M = 129) times that bar.  PC-Relate kinship: at most 0.017 of its bar.
The module's wall time there: 5 s for its 42 device cases (about 1 000 calls); the 6 CPU cases take 3 s.
Value-only defects compiled into scratch copies of the three kernels, each copy run once against this module and the earlier ones.
  k_king, sub-tile j = 1 of the b side left out of the ballot: all 16 cases of test_king_one_missing_call red, first at sample 32.
  k_king, the a side left out of the ballot: those 16, the keep-mask cases and the 4 097-row cases red.
  k_pcrelate, ib1 left out of anyb: all 16 cases with a pair red, first on the diagonal (100, 100), whose b sample sits in sub-tile 1.
  k_project, sample t = 1 left out of the ballot: test_project_one_missing_call red at both shapes.
  k_project, the ring's B1 prefetch with the row mask of the trip before: red at the row outside the model (160, 0), M = 257 only --
  the one defect of the five that no earlier module saw.  The other four also turned cases of test_gpu_king.py, test_gpu_pcrelate.py,
  test_gpu_project.py and test_gpu_exact_pass.py red, through shapes whose last 32-row block holds one or two rows, one-row keep masks and
  the all-missing sample: there the ballot is decided by a handful of calls, but which lane, side or sub-tile decides it is left to the
  seed.  Here every position is placed."""
import functools

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from test_gpu_exact_pass import MISSING, bounds, check_against_bars, exact_pass_model, few_ties, make_inputs
from test_gpu_king import ref_king
from test_gpu_pcrelate import kin_and_bar, ref_pairs, valid_f32

STORES = {"int8": _lib.STORE_INT8, "2bit": _lib.STORE_2BIT}
LAZY_ENV = "GPCA_PROJECT_LAZY_B"


# ---- the shared helper -----------------------------------------------------------------------------------------------------------------------
def lonely(G, row, samples):
    """a copy of the complete matrix G with the call(s) (row, s), s in samples, missing; the rest of the row holds het and hom calls"""
    samples = np.atleast_1d(samples)
    assert not np.any(G == MISSING)
    rest = np.delete(G[row], samples)
    assert np.any(rest == 1) and np.any(rest != 1)
    L = G.copy()
    L[row, samples] = MISSING
    return L


def lower(a, k=-1):
    return a[np.tril_indices(a.shape[0], k)]


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# =============================================================================================================================================
# gpca_king
# =============================================================================================================================================
KING_M, KING_N = 200, 257
KING_ROWS = [0, 15, 16, 31, 32, 63, 64, KING_M - 1]
KING_SAMPLES = [0, 31, 32, 63, 64, 95, 96, 127, 128, KING_N - 1]
KING_PAIRS = [(100, 5), (40, 10), (32, 31), (128, 127), (256, 0), (200, 140)]
KING_PAIR_ROWS = [16, KING_M - 1]
KING_KEEP_ROW, KING_KEEP_SAMPLES = 37, [70, 200]


@functools.lru_cache(maxsize=None)
def king_clean(M):
    rng = np.random.default_rng(7000 + M)
    p = rng.uniform(0.25, 0.5, size=(M, 1))
    G = (rng.random((M, KING_N)) < p).astype(np.int8) + (rng.random((M, KING_N)) < p).astype(np.int8)
    return frozen(G)[0]


def king_keeps(M, row):
    """[(name, keep, the result must be the clean matrix's)]"""
    only = np.zeros(M, np.uint8); only[row] = 1
    alone = np.ones(M, np.uint8); alone[row // 32 * 32:row // 32 * 32 + 32] = 0; alone[row] = 1
    out = np.ones(M, np.uint8); out[row] = 0
    return [("the only kept row", only, False), ("alone in its block", alone, False), ("not kept", out, True)]


def king_sums(G, keep=None, drop=None):
    """ref_king restated from the five sums, with one of them left out (drop = "HM", "MH", "MM") or the missing calls of rows that are not
    kept counted (drop = "unkept"); drop = None is ref_king (asserted by the teeth)."""
    kb = np.ones(G.shape[0], bool) if keep is None else np.asarray(keep).astype(bool)
    X = G[kb]
    H, Mi = (X == 1).astype(np.float64), (X == MISSING).astype(np.float64)
    Xs = np.where(X == 0, -1.0, np.where(X == 2, 1.0, 0.0))
    K = float(X.shape[0])
    HH, HM, MH, MM, XX = H.T @ H, H.T @ Mi, Mi.T @ H, Mi.T @ Mi, Xs.T @ Xs
    if drop in ("HM", "MH", "MM"):
        HM, MH, MM = (np.zeros_like(a) if drop == n else a for n, a in (("HM", HM), ("MH", MH), ("MM", MM)))
    het, miss = H.sum(0), Mi.sum(0)
    if drop == "unkept":
        miss = miss + (G[~kb] == MISSING).sum(0)
    nsnp = ((K - miss[:, None]) - miss[None, :]) + MM
    het_ab, het_ba = het[:, None] - HM, het[None, :] - MH
    homhom = ((nsnp - het_ab) - het_ba) + HH
    ibs0 = (homhom - XX) / 2
    mn = np.minimum(het_ab, het_ba)
    num = ((4 * ibs0 + het_ab) + het_ba) - 2 * HH
    with np.errstate(divide="ignore", invalid="ignore"):
        kin = 0.5 - num / (4 * mn)
    kin[mn == 0] = np.nan
    return kin, np.stack([nsnp, HH, ibs0], axis=-1).astype(np.int32)


def same_king(a, b):
    return np.array_equal(lower(a[0]), lower(b[0]), equal_nan=True) and np.array_equal(lower(a[1]), lower(b[1]))


def test_king_teeth():
    G = king_clean(KING_M)
    everything = np.ones(KING_M, np.uint8)
    some = everything.copy(); some[::5] = 0
    for keep in (everything, some):                                     # the clean matrix: the restatement is ref_king, no mutant moves it
        ref = ref_king(G, keep)
        for drop in (None, "HM", "MH", "MM", "unkept"):
            assert same_king(king_sums(G, keep, drop), ref), drop
    moved = {"HM": 0, "MH": 0, "MM": 0}
    for row in KING_ROWS:
        for s in KING_SAMPLES:
            L = lonely(G, row, s)
            ref = ref_king(L, everything)
            assert same_king(king_sums(L, everything), ref) and not same_king(ref, ref_king(G, everything))
            # H_a M_b lives below the diagonal when a row-side sample a > s is heterozygous there, M_a H_b when a b < s is
            hm, mh = not same_king(king_sums(L, everything, "HM"), ref), not same_king(king_sums(L, everything, "MH"), ref)
            assert hm == (s < KING_N - 1) and mh == (s > 0), (row, s)
            assert same_king(king_sums(L, everything, "MM"), ref)       # (one call alone: M M^T is on the diagonal only)
            moved["HM"] += hm; moved["MH"] += mh
    for row in KING_PAIR_ROWS:
        for pair in KING_PAIRS:
            L = lonely(G, row, pair)
            ref = ref_king(L, everything)
            mm = not same_king(king_sums(L, everything, "MM"), ref)
            assert mm, (row, pair)
            moved["MM"] += mm
    print("lonely cases each mutant moves:", moved)
    for s in KING_KEEP_SAMPLES:                                         # a missing call on a row that is not kept, counted
        L = lonely(G, KING_KEEP_ROW, s)
        for name, keep, as_clean in king_keeps(KING_M, KING_KEEP_ROW):
            ref = ref_king(L, keep)
            assert same_king(ref, ref_king(G, keep)) == as_clean, name
            assert same_king(king_sums(L, keep, "unkept"), ref) == (not as_clean), name


def king_device(e, G, keep):
    e.upload_genotypes_i8(G)
    M = G.shape[0]
    e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), keep)
    return e.king(rows=(0, G.shape[1]), counts=True)


def king_check(got, G, keep, what):
    kin, cnt = got
    ref, rcnt = ref_king(G, keep)
    assert np.array_equal(cnt, lower(rcnt)), what
    assert np.array_equal(kin, lower(ref), equal_nan=True), what


@pytest.mark.gpu
@pytest.mark.parametrize("store", list(STORES))
@pytest.mark.parametrize("row", KING_ROWS)
def test_king_one_missing_call(store, row):
    G = king_clean(KING_M)
    keep = np.ones(KING_M, np.uint8)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        king_check(king_device(e, G, keep), G, keep, f"king {store} clean")
        for s in KING_SAMPLES:
            L = lonely(G, row, s)
            king_check(king_device(e, L, keep), L, keep, f"king {store} lonely ({row}, {s})")
        if row in KING_PAIR_ROWS:
            for pair in KING_PAIRS:
                L = lonely(G, row, pair)
                king_check(king_device(e, L, keep), L, keep, f"king {store} lonely ({row}, {pair})")


@pytest.mark.gpu
@pytest.mark.parametrize("store", list(STORES))
def test_king_one_missing_call_under_keep_masks(store):
    G = king_clean(KING_M)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        for s in KING_KEEP_SAMPLES:
            L = lonely(G, KING_KEEP_ROW, s)
            for name, keep, as_clean in king_keeps(KING_M, KING_KEEP_ROW):
                got = king_device(e, L, keep)
                king_check(got, L, keep, f"king {store} lonely ({KING_KEEP_ROW}, {s}) {name}")
                clean = king_device(e, G, keep)
                same = np.array_equal(got[0], clean[0], equal_nan=True) and np.array_equal(got[1], clean[1])
                assert same == as_clean, name


@pytest.mark.gpu
@pytest.mark.parametrize("store", list(STORES))
def test_king_one_missing_call_in_the_last_block_of_4097_rows(store):
    M = 4097
    G = king_clean(M)
    keep = np.ones(M, np.uint8)
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        for s in (0, 130, KING_N - 1):
            L = lonely(G, M - 1, s)
            king_check(king_device(e, L, keep), L, keep, f"king {store} M={M} lonely ({M - 1}, {s})")


# =============================================================================================================================================
# gpca_project
# =============================================================================================================================================
PRJ_N, PRJ_K = 257, 33
PRJ_SHAPES = [(257, 4), (129, 0)]                                       # (M, gtt_waves): 3 trips in one chunk; two one-trip chunks
PRJ_SAMPLES = [0, 1, 62, 63, 64, PRJ_N - 1]
PRJ_MODES = {"int8": (_lib.STORE_INT8, 4), "2bit": (_lib.STORE_2BIT, 3)}
# lonely calls in a row taken out of the model: a first-trip block, then every slot of the ring in a later trip (rows past M are skipped)
PRJ_OUTSIDE = [(32, 63), (128, 64), (160, 0), (192, 1), (224, PRJ_N - 1)]


def prj_rows(M):
    return sorted({r for r in (0, 15, 16, 31, 32, 64, 96, 127, 128, 160, M - 1) if r < M})


@functools.lru_cache(maxsize=None)
def prj_clean(M):
    """(G complete, mu, sigma, W) -- make_inputs of test_gpu_exact_pass.py without a missing call"""
    return frozen(*make_inputs(M, PRJ_N, PRJ_K, 0.0, "generic", seed=9000 + M))


@functools.lru_cache(maxsize=None)
def prj_clean_model(M, nd):
    return exact_pass_model(*prj_clean(M), nd)


def drop_correction(m_lonely, m_clean):
    """the model's Y with every b o W correction of the lonely matrix left out (Yint_b of the complete matrix: 0), recombined as the model
    does; on the complete matrix itself this is the model"""
    ld = np.longdouble
    Y = (m_lonely["sa"].astype(ld)[None, :] * m_lonely["Yia"].astype(ld) + m_lonely["c"].astype(ld)[None, :]) \
        - m_lonely["sb"].astype(ld)[None, :] * m_clean["Yib"].astype(ld)
    return Y.astype(np.float64)


@pytest.mark.parametrize("nd", [3, 4])
@pytest.mark.parametrize("M,gtt_waves", PRJ_SHAPES)
def test_project_teeth(M, gtt_waves, nd):
    G, mu, sigma, W = prj_clean(M)
    mc = prj_clean_model(M, nd)
    assert mc["digits_ok"] and few_ties(mc) and not np.any(mc["Yib"]) and np.all(mc["used"] == M)
    assert np.array_equal(drop_correction(mc, mc), mc["Y"])             # the mutants leave the clean matrix alone
    worst = np.inf
    for row in prj_rows(M):
        for s in PRJ_SAMPLES:
            m = exact_pass_model(lonely(G, row, s), mu, sigma, W, nd)
            bar, _ = bounds(m, True)
            d = np.abs(drop_correction(m, mc) - m["Y"])
            assert not np.any(d[np.arange(PRJ_N) != s]), (row, s)
            assert not np.any(d[s][bar[s] == 0])                        # (the all-zero column of W: nothing to correct)
            f = float(np.max(d[s][bar[s] > 0] / bar[s][bar[s] > 0]))
            worst = min(worst, f)
            assert f > 1.0, f"M={M} nd={nd} ({row}, {s}): a dropped correction stays inside the bar ({f:.3g} of it)"
            assert m["used"][s] == M - 1 and np.array_equal(np.delete(m["used"], s), np.delete(mc["used"], s))    # the count mutant: used of the clean matrix
    print(f"M={M} nd={nd}: the dropped correction of a lonely call is at least {worst:.3g} of the bar against the model")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(PRJ_MODES))
@pytest.mark.parametrize("M,gtt_waves", PRJ_SHAPES)
def test_project_one_missing_call(monkeypatch, mode, M, gtt_waves):
    store, nd = PRJ_MODES[mode]
    G, mu, sigma, W = prj_clean(M)
    worst = 0.0
    with gpca.GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=store, gtt_waves=gtt_waves) as e:
        def run(Gx, Wx, lazy):
            monkeypatch.setenv(LAZY_ENV, str(lazy))
            e.upload_genotypes_i8(Gx)
            return e.project(mu, sigma, Wx)

        clean = run(G, W, 0)
        mc, _, _ = check_against_bars(clean[0], G, mu, sigma, W, nd, True, f"project {mode} M={M} clean")
        assert np.array_equal(clean[1], mc["used"]) and np.all(clean[1] == M)
        for row in prj_rows(M):
            for s in PRJ_SAMPLES:
                what = f"project {mode} M={M} gtt_waves={gtt_waves} lonely ({row}, {s})"
                L = lonely(G, row, s)
                sc, used = run(L, W, 0)
                m, fm, _ = check_against_bars(sc, L, mu, sigma, W, nd, True, what)
                worst = max(worst, fm)
                assert np.array_equal(used, m["used"]) and used[s] == M - 1, what
                scl, usedl = run(L, W, 1)
                assert np.array_equal(scl, sc) and np.array_equal(usedl, used), what + f": {LAZY_ENV}=1 moved a bit"
        for row, s in PRJ_OUTSIDE:                                      # a row outside the model: its missing call changes nothing
            if row >= M:
                continue
            Wo = W.copy(); Wo[row] = 0
            for lazy in (0, 1):
                ref = run(G, Wo, lazy)
                got = run(lonely(G, row, s), Wo, lazy)
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.all(got[1] == M - 1), (row, s, lazy)
    print(f"project {mode} M={M}: largest fraction of the bar against the model over the lonely cases = {worst:.3g}")


# =============================================================================================================================================
# gpca_pcrelate: the pair count
# =============================================================================================================================================
PCR_M, PCR_N, PCR_TAU = 330, 257, 0.05
PCR_KEEP = np.ones(PCR_M, np.uint8); PCR_KEEP[10::11] = 0
PCR_K = int(PCR_KEEP.sum())
PCR_KROWS = [0, 7, 8, 15, 16, 255, 256, PCR_K - 1]
PCR_PAIRS = [(100, 5), (40, 10), (130, 140), (5, 10), (32, 31), (64, 63), (128, 127), (256, 0)]
assert PCR_K == 300


@functools.lru_cache(maxsize=None)
def pcr_clean():
    """complete genotypes of one population with row frequencies in [0.2, 0.8]: at P = 0 every mu is half a row mean, inside (tau, 1 - tau)"""
    rng = np.random.default_rng(33)
    p = rng.uniform(0.2, 0.8, size=(PCR_M, 1))
    G = (rng.random((PCR_M, PCR_N)) < p).astype(np.int8) + (rng.random((PCR_M, PCR_N)) < p).astype(np.int8)
    return frozen(G)[0]


def pcr_place(ki, pair):
    return lonely(pcr_clean(), int(np.flatnonzero(PCR_KEEP)[ki]), pair)


def nsnp_without_the_product(Gk, mu32, tau):
    """the mutant of ref_pairs' count: K - inv_a - inv_b, the product of the invalid indicators left out"""
    inv = (~valid_f32(Gk, mu32, tau)).sum(0).astype(np.int64)
    return Gk.shape[0] - inv[:, None] - inv[None, :]


def test_pcrelate_teeth():
    def mu_of(Gk):                                                      # (any mu inside (tau, 1 - tau) serves the count: half the row mean)
        return np.repeat((0.5 * np.where(Gk == MISSING, 0, Gk).mean(1, keepdims=True)).astype(np.float32), PCR_N, axis=1)
    kb = PCR_KEEP.astype(bool)
    Gk = pcr_clean()[kb]
    assert np.array_equal(valid_f32(Gk, mu_of(Gk), PCR_TAU), Gk != MISSING)
    assert np.array_equal(nsnp_without_the_product(Gk, mu_of(Gk), PCR_TAU), ref_pairs(Gk, mu_of(Gk), PCR_TAU)[2])
    assert np.all(ref_pairs(Gk, mu_of(Gk), PCR_TAU)[2] == PCR_K)
    for ki in PCR_KROWS:
        for a, b in PCR_PAIRS:
            Lk = pcr_place(ki, (a, b))[kb]
            assert np.array_equal(valid_f32(Lk, mu_of(Lk), PCR_TAU), Lk != MISSING) and (Lk[ki] == MISSING).sum() == 2
            ns, mut = ref_pairs(Lk, mu_of(Lk), PCR_TAU)[2], nsnp_without_the_product(Lk, mu_of(Lk), PCR_TAU)
            assert ns[a, b] == PCR_K - 1 and mut[a, b] == PCR_K - 2 and ns[a, a] == PCR_K - 1 and mut[a, a] == PCR_K - 2
            differ = ns != mut
            assert differ.sum() == 4 and differ[a, b] and differ[b, a] and differ[a, a] and differ[b, b]


@pytest.mark.gpu
@pytest.mark.parametrize("store", list(STORES))
@pytest.mark.parametrize("ki", PCR_KROWS + [None])
def test_pcrelate_pair_count_with_one_pair_of_missing_calls(store, ki):
    kb = PCR_KEEP.astype(bool)
    worst = 0.0
    with gpca.GpcaEngine(storage=STORES[store]) as e:
        for pair in (PCR_PAIRS if ki is not None else [None]):
            G = pcr_clean() if ki is None else pcr_place(ki, pair)
            what = f"pcrelate {store} kept row {ki} samples {pair}"
            e.upload_genotypes_i8(G)
            e.set_standardization(np.ones(PCR_M, np.float32), np.ones(PCR_M, np.float32), PCR_KEEP)
            mu, _ = e.pcrelate_isaf(None)
            kin, ns = e.pcrelate(None, maf_bound=PCR_TAU, rows=(0, PCR_N), nsnp=True)
            Gk = G[kb]
            assert mu.shape == Gk.shape and np.array_equal(valid_f32(Gk, mu, PCR_TAU), Gk != MISSING), what + ": validity is not observedness"
            num, den, nsnp, anum = ref_pairs(Gk, mu, PCR_TAU)
            assert np.array_equal(ns, lower(nsnp, 0)), what
            if ki is not None:
                a, b = max(pair), min(pair)
                assert nsnp[a, b] == PCR_K - 1 and nsnp[a, a] == PCR_K - 1 and nsnp[b, b] == PCR_K - 1
                assert not np.array_equal(lower(nsnp_without_the_product(Gk, mu, PCR_TAU), 0), ns), what
            rk, bar = kin_and_bar(num, den, nsnp, anum)
            rk, bar = lower(rk, 0), lower(bar, 0)
            assert not np.any(np.isnan(rk)) and not np.any(np.isnan(kin)), what
            err = np.abs(kin - rk)
            worst = max(worst, float(np.max(err / bar)))
            assert np.all(err <= bar), what
    print(f"pcrelate {store} kept row {ki}: largest fraction of the kinship bar = {worst:.3g}")
