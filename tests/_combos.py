"""Pairwise-covering case tables that cross the edge axes of the band kernels, and the builders that turn a case into inputs.

tests/_edges.py walks every axis on its own.  The two tables below cross them: every value of every axis meets every value of every
other axis in at least one case (``pairwise``: a greedy covering array; pairs, not triples).  ROW_TABLE is for the features whose band
is a range of kept rows (group_counts, f2_blocks, sample_counts, roh, ld_score; K is given in units of the feature's row extent R),
SAMPLE_TABLE for the ones whose band is a range of samples of the lower triangle (king, grm).  ``FEATURES`` holds, per feature, how a
case becomes inputs (``build``), what the feature's own model expects for them (``expect``: used by the teeth of
test_edge_combos_table.py, numpy only) and how the device is held to it (``run``: the feature module's own checker).  The feature
modules are imported inside those functions, so the tables themselves need numpy alone.

Where a shape cannot hold a band class ``band_for`` returns the nearest legal band and the pair is listed in EXEMPT.  A case whose
data cannot bite at seed 0 (all-zero counts at one sample, say) names another seed in RESEED; the case itself stays in the table."""
import random

import numpy as np

MISSING = -127
KEEPS = ["all", "holes", "first", "last"]
MISSES = ["none", "2 %", "special"]
STORES = ["int8", "2bit"]
ROW_BANDS = ["full", "head", "tail", "inner", "one"]
SAMPLE_BANDS = ROW_BANDS + ["lastrow"]
ROW_AXES = [("N", [1, 17, 64, 255, 257, 1025]), ("K", ["1", "R-1", "R", "R+1", "2R+1"]), ("keep", KEEPS), ("band", ROW_BANDS),
            ("store", STORES), ("miss", MISSES), ("x", [0, 1, 2])]
SAMPLE_AXES = [("N", [2, 64, 127, 128, 129, 257, 1025]), ("K", [1, 33, 4097]), ("keep", KEEPS), ("band", SAMPLE_BANDS),
               ("store", STORES), ("miss", MISSES)]
# the pairs a case cannot hold as named: one kept row has one band, (0, 1); two samples have no band strictly inside (0, 2)
EXEMPT = {"row": [(("K", "1"), ("band", b)) for b in ("head", "tail", "inner", "one")],
          "sample": [(("N", 2), ("band", "inner"))]}


def pairwise(axes, seed):
    """a list of dicts over `axes` = [(name, values)] in which every two values of two different axes occur together at least once.
    Greedy: each new case is the best of 40 candidates, a candidate takes the axes in a random order and gives each the value that
    covers the most pairs still open against the values already chosen (ties by the random order).  Deterministic in `seed`."""
    rng = random.Random(seed)
    names = [n for n, _ in axes]
    vals = dict(axes)
    todo = {((a, u), (b, v)) for i, a in enumerate(names) for b in names[i + 1:] for u in vals[a] for v in vals[b]}
    key = lambda a, u, b, v: ((a, u), (b, v)) if names.index(a) < names.index(b) else ((b, v), (a, u))
    cases = []
    while todo:
        best, best_new = None, -1
        for _ in range(40):
            first = sorted(todo, key=repr)[rng.randrange(len(todo))]          # (a candidate starts from a pair that is still open)
            case = dict(first)
            order = [n for n in names if n not in case]
            rng.shuffle(order)
            for a in order:
                pool = list(vals[a])
                rng.shuffle(pool)
                case[a] = max(pool, key=lambda u: sum(key(a, u, b, v) in todo for b, v in case.items()))
            new = sum(key(a, case[a], b, case[b]) in todo for i, a in enumerate(names) for b in names[i + 1:])
            if new > best_new:
                best, best_new = case, new
        cases.append({n: best[n] for n in names})
        todo -= {key(a, best[a], b, best[b]) for i, a in enumerate(names) for b in names[i + 1:]}
    return cases


def pairs_of(cases, axes):
    """the set of ((axis, value), (axis, value)) pairs, in axis order, that `cases` hold"""
    names = [n for n, _ in axes]
    return {((a, c[a]), (b, c[b])) for c in cases for i, a in enumerate(names) for b in names[i + 1:]}


ROW_TABLE = pairwise(ROW_AXES, seed=1)
SAMPLE_TABLE = pairwise(SAMPLE_AXES, seed=2)


def case_id(c):
    return "-".join(str(v).replace(" ", "") for v in c.values())


def k_of(c, R):
    """the kept rows of a case: a row-band case names them in units of the feature's row extent R"""
    k = c["K"]
    return k if isinstance(k, int) else {"1": 1, "R-1": R - 1, "R": R, "R+1": R + 1, "2R+1": 2 * R + 1}[k]


# ---------------------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------------------
def keep_for(K, pattern):
    """(M, keep uint8 [M]) with exactly K kept rows.  all: M = K.  holes: an irregular two in three (of every three rows one is
    dropped, at a position that moves), so the kept-row list is not the identity and not a stride.  first: the first 32-row block
    dropped.  last: the kept rows first, then nothing up to the 32-row boundary and a partial block of 17 rows: the whole last
    block is dropped, as _edges.edge_keeps does, and M is not a multiple of 32."""
    if pattern == "all":
        keep = np.ones(K, np.uint8)
    elif pattern == "holes":
        keep = np.ones(3 * ((K + 1) // 2), np.uint8)
        t = np.arange(keep.size // 3)
        keep[3 * t + (t * t + t // 3) % 3] = 0
        keep = keep[:np.flatnonzero(np.cumsum(keep) == K)[0] + 1]
    elif pattern == "first":
        keep = np.concatenate([np.zeros(32, np.uint8), np.ones(K, np.uint8)])
    elif pattern == "last":
        keep = np.zeros(-(-K // 32) * 32 + 17, np.uint8)
        keep[:K] = 1
        assert not keep[(keep.size - 1) // 32 * 32:].any()
    else:
        raise ValueError(pattern)
    assert int(keep.sum()) == K
    return keep.size, keep


def band_for(extent, cls, tile=32):
    """[r0, r1) of `extent` rows (tile = 32) or samples (tile = 128): full; head (0, s); tail (s, extent); inner (a, b), a and b in
    different tiles where the extent allows; one (a, a + 1); lastrow (extent - 1, extent).  s, a and b are no multiple of the tile
    and lie strictly inside.  Where the extent cannot hold the class (EXEMPT) the nearest legal band comes back."""
    off = lambda v: v - 1 if v % tile == 0 and v > 1 else v
    if cls == "full" or extent == 1:
        return 0, extent
    if cls == "head":
        return 0, off(max(1, 2 * extent // 3))
    if cls == "tail":
        return off(max(1, extent // 3)), extent
    if cls == "inner":
        if extent < 3:
            return extent - 1, extent
        a = off(max(1, extent // 4))
        return a, max(a + 1, min(extent - 1, off(extent - extent // 4)))
    if cls == "one":
        a = max(1, extent // 2)
        while a > 1 and (a % tile == 0 or (a + 1) % tile == 0):
            a -= 1
        return a, a + 1
    if cls == "lastrow":
        return extent - 1, extent
    raise ValueError(cls)


def missing_for(G, cls, keep=None, seed=0):
    """a copy of G (which holds no missing call) with the class's missing calls.  none.  2 %: at random.  special: one sample
    (N // 3) missing on every row and one kept row (the middle one) missing at every sample."""
    G = G.copy()
    assert not (G == MISSING).any()
    if cls == "2 %":
        G[np.random.default_rng([97, seed, G.shape[0], G.shape[1]]).random(G.shape) < 0.02] = MISSING
        if not (G == MISSING).any():
            G[G.shape[0] // 2, G.shape[1] // 2] = MISSING
    elif cls == "special":
        kr = np.arange(G.shape[0]) if keep is None else np.flatnonzero(keep)
        G[:, G.shape[1] // 3] = MISSING
        G[kr[len(kr) // 2], :] = MISSING
    elif cls != "none":
        raise ValueError(cls)
    return G


def band_keep(keep, band):
    """the keep mask that holds the kept rows [band[0], band[1]) of `keep` only"""
    out = np.zeros_like(keep)
    out[np.flatnonzero(keep)[band[0]:band[1]]] = 1
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the features: build(case, seed) -> inputs; expect(inp, G, keep, band) -> arrays of the feature's own model; run(e, inp, mp)
# ---------------------------------------------------------------------------------------------------------------------------------
def _shape(c, R, tile=32):
    """what every feature starts from: K, (M, keep), the band over the kept rows (row tables) or the samples (sample table)"""
    K = k_of(c, R) if R else c["K"]
    M, keep = keep_for(K, c["keep"])
    band = band_for(K, c["band"]) if R else band_for(c["N"], c["band"], 128)
    return dict(case=c, K=K, M=M, N=c["N"], keep=keep, band=band, store=c["store"])


def _all_missing(inp):
    if inp["case"]["miss"] == "special" and (inp["K"] == 1 or inp["N"] == 1):
        return "the one kept row (the one sample) is the special one: every call that counts is missing, whatever the seed"
    return None


def _standardize(e, keep):
    M = keep.size
    e.set_standardization(np.ones(M, np.float32), np.ones(M, np.float32), keep)


class GroupCounts:
    name, R, table = "group_counts", 128, "row"                               # kGcRows (plan_math.h)
    P = [2, 33, 64]

    def build(self, c, seed):
        import test_gpu_group_counts as t
        inp = _shape(c, self.R)
        inp["P"] = self.P[c["x"]]
        G, inp["group"] = t.make(inp["M"], inp["N"], inp["P"], seed=[5, seed] + list(map(ord, case_id(c))), miss=0.0)
        inp["G"] = missing_for(G, c["miss"], inp["keep"], seed)
        return inp

    def expect(self, inp, G, keep, band):
        import test_gpu_group_counts as t
        return (t.model(G, inp["group"], inp["P"], keep)[band[0]:band[1]],)

    def run(self, e, inp, mp):
        import test_gpu_group_counts as t
        t.load(e, inp["G"], inp["keep"])
        got = e.group_counts(inp["group"], inp["P"], rows=inp["band"])
        want, = self.expect(inp, inp["G"], inp["keep"], inp["band"])
        assert got.dtype == np.uint32 and got.shape == want.shape and np.array_equal(got, want), label(inp)

    def toothless(self, inp):
        return _all_missing(inp)


class F2Blocks(GroupCounts):
    name, R = "f2_blocks", 256                                                # kFbRun
    P = [2, 24, 64]

    def build(self, c, seed):
        from test_gpu_f2_blocks import runs
        inp = GroupCounts.build(self, c, seed)
        rows = inp["band"][1] - inp["band"][0]
        if c["x"] == 0:
            block = np.zeros(rows, np.int32)                                  # one block
        elif c["x"] == 1:
            block = runs(rows, 7)                                             # runs of 7 rows, some rows in no block
            block[np.random.default_rng([6, seed, rows]).random(rows) < 0.2] = -1
            if rows > 2:
                block[rows // 2] = -1
        else:
            block = np.arange(rows, dtype=np.int32)                           # every row its own block
        inp["block"], inp["B"] = block, int(block.max(initial=0)) + 1
        return inp

    def expect(self, inp, G, keep, band):
        import test_gpu_group_counts as g
        from test_gpu_f2_blocks import model_f2
        return model_f2(g.model(G, inp["group"], inp["P"], keep)[band[0]:band[1]], inp["block"], inp["B"])

    def run(self, e, inp, mp):
        import test_gpu_group_counts as g
        from test_gpu_f2_blocks import check
        g.load(e, inp["G"], inp["keep"])
        try:
            check(e, inp["G"], inp["group"], inp["P"], inp["block"], inp["B"], keep=inp["keep"], rows=inp["band"])
        except AssertionError as err:
            raise AssertionError(f"{label(inp)}: {err}") from err

    def toothless(self, inp):
        if inp["N"] == 1:
            return "one sample fills one group: no pair of groups has a call on any row, acc and cnt are zero whatever the data"
        return _all_missing(inp)


class SampleCounts:
    name, R, table = "sample_counts", 64, "row"
    X = [(None, False), (2, True), (7, True)]                                 # (GPCA_SAMPLE_COUNTS_SPLITS, weights)

    def build(self, c, seed):
        import test_gpu_sample_counts as t
        inp = _shape(c, self.R)
        inp["splits"], weighted = self.X[c["x"]]
        G, q = t.make(inp["M"], inp["N"], seed=[7, seed] + list(map(ord, case_id(c))), miss=0.0)
        rows = inp["band"][1] - inp["band"][0]
        inp["q"] = q[:rows].copy() if weighted else None                      # one weight per row of the band; q[0] = 2^30
        inp["G"] = missing_for(G, c["miss"], inp["keep"], seed)
        return inp

    def expect(self, inp, G, keep, band):
        import test_gpu_sample_counts as t
        keep = np.ones(G.shape[0], np.uint8) if keep is None else keep
        counts, qs = t.model(G, inp["q"], band_keep(keep, band))
        return (counts,) if qs is None else (counts, qs)

    def run(self, e, inp, mp):
        import test_gpu_sample_counts as t
        if inp["splits"] is None:
            mp.delenv("GPCA_SAMPLE_COUNTS_SPLITS", raising=False)
        else:
            mp.setenv("GPCA_SAMPLE_COUNTS_SPLITS", str(inp["splits"]))        # (the library reads it per call)
        t.load(e, inp["G"], inp["keep"])
        t.check(e, inp["G"], inp["q"], inp["keep"], rows=inp["band"], what=label(inp))

    def toothless(self, inp):
        return _all_missing(inp)


class Roh:
    name, R, table = "roh", 64, "row"
    X = [(5, None), (50, 3), (64, 7)]                                         # (window_snp, GPCA_ROH_SPLITS)

    def build(self, c, seed):
        import test_gpu_roh as t
        inp = _shape(c, self.R)
        W, inp["splits"] = self.X[c["x"]]
        K = inp["K"]
        G = t.make(inp["M"], inp["N"], 0.25 if W == 5 else 0.02, 0.0, seed=[8, seed] + list(map(ord, case_id(c))))
        inp["G"] = missing_for(G, c["miss"], inp["keep"], seed)
        inp["brk"] = t.breaks(K, dom=[K // 3], cut=[K // 2])                  # a domain start and a cut, over all kept rows
        inp["p"] = t.P(W=W, H=1, M=min(W, 5), num=1, den=20, min_snp=3)
        return inp

    def expect(self, inp, G, keep, band):
        import test_gpu_roh as t
        return t.model(G, inp["brk"][inp["band"][0]:inp["band"][1]], inp["p"], keep, band)

    def run(self, e, inp, mp):
        import test_gpu_roh as t
        if inp["splits"] is None:
            mp.delenv("GPCA_ROH_SPLITS", raising=False)
        else:
            mp.setenv("GPCA_ROH_SPLITS", str(inp["splits"]))
        t.load(e, inp["G"], inp["keep"])
        r0, r1 = inp["band"]
        t.check(e, inp["G"], inp["brk"][r0:r1], inp["p"], keep=inp["keep"], rows=inp["band"], what=label(inp))

    def toothless(self, inp):
        r0, r1 = inp["band"]
        starts = [0] + [j - r0 for j in np.flatnonzero(inp["brk"] & 1) if r0 < j < r1] + [r1 - r0]
        if max(b - a for a, b in zip(starts[:-1], starts[1:])) < inp["p"]["W"]:
            return "no domain of the band holds a window: there is no record whatever the data (the device must report none)"
        return None


class LdScore:
    name, R, table = "ld_score", 64, "row"
    X = [1, 63, 200]                                                          # the window in rows, uniform; wmax = the window

    def build(self, c, seed):
        import test_gpu_ld_score as t
        inp = _shape(c, self.R)
        inp["w"] = self.X[c["x"]]
        G = t.genotypes(inp["M"], inp["N"], seed=1000 * seed + sum(map(ord, case_id(c))), miss=0.0)
        inp["G"] = missing_for(G, c["miss"], inp["keep"], seed)
        inp["we"] = t.uniform_windows(inp["K"], inp["w"])
        return inp

    def expect(self, inp, G, keep, band):
        import test_gpu_ld_score as t
        keep = np.ones(G.shape[0], np.uint8) if keep is None else keep
        we = t.uniform_windows(int(keep.sum()), inp["w"])                     # (every row kept: more rows, the same band indices)
        return t.model_a(G, keep, we[band[0]:band[1]], inp["w"], band[0], band[1], True)

    def run(self, e, inp, mp):
        import test_gpu_ld_score as t
        t.open_handle(e, inp["G"], inp["keep"])
        try:
            t.check(e, inp["G"], inp["keep"], inp["we"], inp["w"], band=inp["band"])
        except AssertionError as err:
            raise AssertionError(f"{label(inp)}: {err}") from err

    def toothless(self, inp):
        if inp["K"] == 1 or inp["N"] <= 2:
            return "one kept row has no partner and n <= 2 skips every pair: score and partners are zero whatever the data"
        return _all_missing(inp)


def _tri_rows(N, band, strict):
    a, b = np.tril_indices(N, -1 if strict else 0)
    sel = (a >= band[0]) & (a < band[1])
    return a[sel], b[sel]


class King:
    name, R, table = "king", None, "sample"
    _memo = None

    def build(self, c, seed):
        import test_gpu_king as t
        inp = _shape(c, None)
        G = t.genotypes(inp["M"], inp["N"], seed=[9, seed] + list(map(ord, case_id(c))))
        inp["G"] = missing_for(G, c["miss"], inp["keep"], seed)
        return inp

    def full(self, inp, G, keep):
        """(counts, kinship) of every pair; the last one is remembered (the teeth slice it several times)"""
        import test_gpu_king as t
        if not (self._memo and self._memo[0] is G and self._memo[1] is keep):
            kin, cnt = t.ref_king(G, keep)
            self._memo = (G, keep, (cnt, kin))
        return self._memo[2]

    def expect(self, inp, G, keep, band):
        """the rows [band) of the full symmetric model (all columns, so that a shifted band has the same shape)"""
        return tuple(x[band[0]:band[1]] for x in self.full(inp, G, keep))

    def run(self, e, inp, mp):
        import genomic_pca_amd as gpca
        e.upload_genotypes_i8(inp["G"])
        e.snp_stats(gpca.QcConfig.none())
        _standardize(e, inp["keep"])
        kin, cnt = e.king(rows=inp["band"], counts=True)
        rcnt, ref = self.full(inp, inp["G"], inp["keep"])
        a, b = _tri_rows(inp["N"], inp["band"], strict=True)
        assert kin.shape == (a.size,) and cnt.shape == (a.size, 3), label(inp)
        assert np.array_equal(cnt, rcnt[a, b]), label(inp)
        assert np.array_equal(kin, ref[a, b], equal_nan=True), label(inp)

    def toothless(self, inp):
        return _all_missing(inp)


class Grm:
    name, R, table = "grm", None, "sample"
    SCALINGS = ("standardized", "centred")
    _memo = None

    def build(self, c, seed):
        inp = _shape(c, None)
        M, N = inp["M"], inp["N"]
        rng = np.random.default_rng([10, seed] + list(map(ord, case_id(c))))
        p = rng.uniform(0.05, 0.5, size=M)                                    # test_gpu_grm_exact's ``generic`` family
        G = (rng.random((M, N)) < p[:, None]).astype(np.int8) + (rng.random((M, N)) < p[:, None]).astype(np.int8)
        inp["mu"], inp["sigma"] = (2 * p).astype(np.float32), np.sqrt(2 * p * (1 - p)).astype(np.float32)
        inp["G"] = missing_for(G, c["miss"], inp["keep"], seed)
        return inp

    def model(self, inp, G, keep, scaling):
        """test_gpu_grm_exact's model of the whole matrix; the last one is remembered (the teeth slice it several times)"""
        from test_gpu_grm_exact import grm_model
        if not (self._memo and self._memo[0] is G and self._memo[1] is keep and self._memo[2] == scaling):
            mdl = grm_model(G, inp["mu"], inp["sigma"], np.ones(G.shape[0], np.uint8) if keep is None else keep, scaling)
            self._memo = (G, keep, scaling, mdl)
        return self._memo[3]

    def expect(self, inp, G, keep, band, scaling="standardized"):
        m = self.model(inp, G, keep, scaling)
        return m.grm[band[0]:band[1]], m.npairs[band[0]:band[1]]

    def run(self, e, inp, mp):
        from test_gpu_grm_exact import _standardize as std, check_device, flush_groups
        e.upload_genotypes_i8(inp["G"])
        std(e, inp["mu"], inp["sigma"], inp["keep"])
        for scaling in self.SCALINGS:
            tri, npt = e.grm(scaling, rows=inp["band"], npairs=True)
            mdl = self.model(inp, inp["G"], inp["keep"], scaling)
            assert check_device(tri, npt, mdl, flush_groups(inp["M"]), (label(inp), scaling), rows=inp["band"]) == "exact"

    def toothless(self, inp):
        return _all_missing(inp)


FEATURES = {f.name: f for f in (GroupCounts(), F2Blocks(), SampleCounts(), Roh(), LdScore(), King(), Grm())}
TABLES = {"row": ROW_TABLE, "sample": SAMPLE_TABLE}
# (feature, index of the case in its table) -> the seed of the case's data, where seed 0 cannot bite (test_edge_combos_table.py)
# (at seed 0 the missing calls of these three fall where the output cannot see them: outside the band, or on a sample without a group)
RESEED = {("group_counts", 2): 1, ("group_counts", 19): 1, ("f2_blocks", 1): 1}


def table_of(feature):
    return TABLES[FEATURES[feature].table]


def build(feature, i):
    """the inputs of case i of the feature's table, at the case's seed"""
    return FEATURES[feature].build(table_of(feature)[i], RESEED.get((feature, i), 0))


def label(inp):
    """what an assertion message says of a case: the shape, the band and the axes"""
    return f"{inp['M']} x {inp['N']} (K = {inp['K']}), band {inp['band']}, {inp['case']}"
