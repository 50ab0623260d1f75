"""The case table of tests/_corr_walk.py, on the CPU: coverage, determinism, the builder's promises, and that the cases can bite.

Coverage: every pair of values of every two axes occurs in some case of the pairwise table; the pairs of EXEMPT occur too and run with
the nearest legal value (module docstring there).  Every forced slot count that is left after NO_FORCE meets every N class and both
corrections.  Every case's inputs are accepted by the null fit (the builder runs gpca_logistic_null per trait: it raises otherwise), the
keep masks hold what they are named for, and the bands lie where they are named.
Bite, on the f64 restatement alone (U, a_j and z from test_gpu_assoc_score.restate / finish instead of the device): a case that forces
s workgroups lists at least 2 s + 1 items even with the cutoff raised by 1e-3 (the device's z comes from an f32 pass: its relative
distance from the restatement's is below 1e-4 at these shapes, test_gpu_assoc_score.py), and every case NO_FORCE names would indeed
list fewer without that margin or is named for a reason that no data can change.
The skip cap of the device module, reference alone: test_gpu_assoc_spa.check_against_restatement may skip an item only where
near_decision fires, at most 2 % of a case's items.  near_decision reads the two support bounds of the reference and nothing else of
it, so they are formed here as spa_reference forms them (the sums of max and min of g~ (1 - mu), -g~ mu), without its root rule: no
case of the table skips more than 2 % of its items before a device sees it."""
import numpy as np
import pytest

import _combos
import _corr_walk as W

IDS = [W.case_id(i) for i in range(len(W.CASES))]


def test_coverage_and_determinism():
    names = [n for n, _ in W.AXES]
    every = {((a, u), (b, v)) for i, (a, va) in enumerate(W.AXES) for b, vb in W.AXES[i + 1:] for u in va for v in vb}
    assert _combos.pairs_of(W.TABLE, W.AXES) == every
    assert all(list(c) == names and all(c[n] in dict(W.AXES)[n] for n in names) for c in W.CASES)
    assert _combos.pairwise(W.AXES, 31) == W.TABLE
    assert len(W.TABLE) <= 56, len(W.TABLE)              # (the product holds 13 824 cases)
    assert all(p in every for p in W.EXEMPT)
    assert len(set(IDS)) == len(IDS)
    print(f"{len(W.TABLE)} table cases and {len(W.EXTRA)} hand-written ones; {len(W.NO_FORCE)} forced counts dropped")


def test_every_forced_count_meets_every_n_class_and_both_corrections():
    seen = set()
    for i in range(len(W.CASES)):
        inp = W.resolve(i)
        if inp["slots"] is not None:
            cls = [k for k, v in W.N_CLASSES.items() if inp["N"] in v]
            assert len(cls) == 1
            seen.add((inp["corr"], cls[0], inp["slots"]))
    want = {(corr, cls, s) for corr in ("spa", "firth") for cls in W.N_CLASSES for s in (1, 2, 3)}
    assert want <= seen, sorted(want - seen)
    assert all(0 <= i < len(W.CASES) and W.CASES[i]["slots"] is not None for i in W.NO_FORCE)


def test_resolved_cases_hold_what_they_name():
    for i in range(len(W.CASES)):
        inp = W.resolve(i)
        c, keep, K, (a, b) = inp["case"], inp["keep"], inp["K"], inp["band"]
        assert keep.shape == (inp["L"],) and inp["L"] == (45 if c["N"] <= 8257 else 12) and K == int(keep.sum()) >= 1
        assert (inp["T"], inp["Pc"]) == W.TPS[c["tp"]] or (c["N"] < 257 and c["tp"] == "1x61" and (inp["T"], inp["Pc"]) == (1, 0))
        assert inp["T"] * (inp["Pc"] + 3) <= 64
        kr = np.flatnonzero(keep)
        if c["keep"] == "all":
            assert K == inp["L"]
        if c["keep"] == "holes":                          # not the identity, and the special rows stay
            assert K < inp["L"] and all(keep[j] for j in (0, 1, 2, 3, 5, 6, 7, inp["L"] - 1)) and np.any(kr[:K] != np.arange(K))
        if c["keep"] == "one":
            assert K == 1 and kr[0] != 0
        assert 0 <= a <= b <= K
        if c["band"] == "full" or (c["band"] == "inner" and K < 3):
            assert (a, b) == (0, K)
        elif c["band"] == "inner":
            assert 0 < a < b < K
        else:
            assert a == b
        assert inp["slots"] in (None, 1, 2, 3) and K * inp["T"] <= 1021     # with the hook unset no workgroup takes a second item


@pytest.mark.parametrize("i", range(len(W.CASES)), ids=IDS)
def test_case_is_accepted_bites_and_keeps_the_skip_cap(i):
    import test_gpu_assoc_firth as tf
    from test_assoc_spa_host import near_decision
    from test_gpu_assoc_spa import operand
    inp = W.build(i)                                      # (the null fit of every trait: raises where it refuses one)
    assert inp["G"].shape == (inp["L"], inp["N"]) and inp["G"].dtype == np.int8 and len(inp["nulls"]) == inp["T"]
    if inp["special"]:
        assert np.all(inp["G"][-1] == -127)               # the row without an observed call is loaded
    r = W.restated(inp)
    loose, tight = W.listed(inp, r), W.listed(inp, r, margin=1e-3)
    s, forced = inp["slots"], inp["case"]["slots"]
    print(f"{IDS[i]}: K = {inp['K']}, {inp['K'] * inp['T']} items, {int(loose.sum())} listed ({int(tight.sum())} with the margin)")
    if s is not None:
        assert int(tight.sum()) >= 2 * s + 1, (IDS[i], int(tight.sum()))
    elif forced is not None:                              # named in NO_FORCE: it could indeed not be relied on
        assert int(tight.sum()) < 2 * forced + 1, (IDS[i], int(tight.sum()), W.NO_FORCE[i])
    if inp["corr"] != "spa":
        return
    Gk = inp["G"][inp["kept"]]
    sm = inp["inc"].astype(bool)
    x, ms, xbar = operand(Gk, inp["inc"], r["flipped"])
    skipped = 0
    for k, t in zip(*np.nonzero(loose)):
        g, mu, Uv, dg = tf.item_inputs(r, x, ms, xbar, sm, inp["nulls"][t], k, t, inp["Pc"])
        p, q = g * (1.0 - mu), -g * mu
        ref = {"hi": float(np.sum(np.maximum(p, q))), "lo": float(np.sum(np.minimum(p, q)))}
        skipped += bool(near_decision(g, mu, Uv, ref, dg))
    assert skipped <= 0.02 * inp["K"] * inp["T"], (IDS[i], skipped)
