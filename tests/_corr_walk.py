"""The case table that crosses the walk edges of the two corrections of the logistic score scan (k_assoc_spa, k_assoc_firth), and the
builder that turns a case into inputs.  tests/test_gpu_assoc_corr_walk.py runs the cases on the device, tests/test_assoc_corr_walk_table.py
holds the table to its promises on the CPU.  The test modules are imported inside the functions: the table itself needs numpy alone.

Axes (``pairwise`` of tests/_combos.py: every value of every axis meets every value of every other axis in some case):
  corr   spa, firth.
  cut    dense (spa_z = 0.5, firth_z = 0: nearly every item is listed), sparse (spa_z = 2, firth_z = the default: the list has holes).
  N      63, 65 (one stage, two), 8191, 8192 (one staging chunk, the last one full), 8193 (a second chunk of one sample), 8257 (a second
         chunk of two stages, 65 real samples), 16385 (a third chunk of one sample), 32769 (a fifth chunk; fewer than 1024 slots).
  tp     (T, Pc) = (1, 0), (2, 3), (21, 0) (the widest item / T decode), (1, 61) (62 entries of sa).
  slots  GPCA_ASP_SLOTS unset, 1, 2, 3.
  keep   all; holes (the special rows stay); one (a single kept row, not row 0).
  band   full; inner (starts past kept row 0, ends before the last kept row); empty.
  eng    int8, 2bit, f32 (int8 storage on a PREC_F32_MFMA handle).
What a case cannot hold as named (EXEMPT; the case stays in the table with the nearest legal value): (1, 61) below N = 257 runs as
(1, 0), as in the two modules whose inputs these are; one kept row has no inner band and runs the full one.
A forced slot count must bite: with s workgroups at least 2 s + 1 items are corrected, so that some workgroup takes a third item.
Where a case cannot (too few items above a sparse cutoff, one kept row with one trait) the forced count is dropped for that case,
NO_FORCE names the case and the case id says ``slotsN-dropped``; EXTRA holds hand-written cases that put back what the drops take
out of "every forced count meets every N class and both corrections".

Rows: 45 loaded rows up to N = 8257 and 12 from N = 16385 on, taken from the 130 rows of the existing modules' inputs: the first
L - 1 and row 65, the one without an observed call, so that every special row (0 flipped, 1 collinear with covariate 0, 2 monomorphic,
3 with s1 = n_obs, 5 .. 7 Firth's singletons and all-cases carriers) is loaded."""
import numpy as np

from _combos import pairwise

NS = [63, 65, 8191, 8192, 8193, 8257, 16385, 32769]
TPS = {"1x0": (1, 0), "2x3": (2, 3), "21x0": (21, 0), "1x61": (1, 61)}
AXES = [("corr", ["spa", "firth"]), ("cut", ["dense", "sparse"]), ("N", NS), ("tp", list(TPS)), ("slots", [None, 1, 2, 3]),
        ("keep", ["all", "holes", "one"]), ("band", ["full", "inner", "empty"]), ("eng", ["int8", "2bit", "f32"])]
EXEMPT = [(("N", n), ("tp", "1x61")) for n in (63, 65)] + [(("keep", "one"), ("band", "inner"))]
CUTOFF = {("spa", "dense"): 0.5, ("spa", "sparse"): 2.0, ("firth", "dense"): 0.0, ("firth", "sparse"): 1.959964}
ALL_MISSING = 65                                          # M_ROWS // 2 of the 130-row inputs
N_CLASSES = {"one chunk": (63, 65, 8191, 8192), "two chunks": (8193, 8257), "three chunks": (16385,), "five chunks, 1022 slots": (32769,)}

TABLE = pairwise(AXES, seed=31)
# hand-written cases (module docstring): a forced count for the (corr, N class) pairs whose table cases had to drop theirs
EXTRA = [
    dict(corr="spa", cut="dense", N=8257, tp="2x3", slots=1, keep="holes", band="inner", eng="f32"),
    dict(corr="spa", cut="dense", N=8193, tp="21x0", slots=2, keep="holes", band="full", eng="int8"),
    dict(corr="spa", cut="dense", N=8257, tp="1x61", slots=3, keep="all", band="inner", eng="2bit"),
    dict(corr="spa", cut="dense", N=16385, tp="21x0", slots=2, keep="holes", band="full", eng="int8"),
    dict(corr="spa", cut="dense", N=16385, tp="2x3", slots=3, keep="all", band="inner", eng="f32"),
    dict(corr="spa", cut="dense", N=32769, tp="21x0", slots=2, keep="all", band="full", eng="2bit"),
    dict(corr="spa", cut="dense", N=32769, tp="2x3", slots=3, keep="holes", band="inner", eng="2bit"),
    dict(corr="firth", cut="dense", N=8192, tp="2x3", slots=3, keep="all", band="inner", eng="f32"),
    dict(corr="firth", cut="dense", N=16385, tp="1x0", slots=1, keep="all", band="inner", eng="int8"),
    dict(corr="firth", cut="dense", N=16385, tp="21x0", slots=2, keep="holes", band="full", eng="f32"),
    dict(corr="firth", cut="dense", N=16385, tp="2x3", slots=3, keep="holes", band="inner", eng="2bit"),
    dict(corr="firth", cut="dense", N=32769, tp="1x61", slots=1, keep="holes", band="inner", eng="int8"),
    dict(corr="firth", cut="dense", N=32769, tp="21x0", slots=2, keep="all", band="inner", eng="f32"),
]
CASES = TABLE + EXTRA
# index in CASES -> why the case's forced slot count cannot bite (test_assoc_corr_walk_table.py holds every other forced case to
# 2 s + 1 corrected items on the f64 restatement, with a margin on the cutoff)
_FEW = "a sparse cutoff over a few dozen items lists fewer than 2 s + 1 of them"
_ONE = "one kept row with at most two traits has fewer than 2 s + 1 items"
NO_FORCE = {0: _FEW, 5: _ONE, 6: _ONE, 15: _ONE, 16: _ONE, 17: _FEW, 20: _ONE, 23: _FEW, 25: _ONE, 29: _FEW, 32: _ONE}


def loaded_rows(N):
    return 45 if N <= 8257 else 12


def resolve(i):
    """case i of CASES as it runs: (T, Pc), the forced slot count or None, the keep mask over the loaded rows, the band over the kept rows"""
    c = CASES[i]
    N = c["N"]
    T, Pc = TPS[c["tp"]]
    if Pc == 61 and N < 257:
        T, Pc = 1, 0
    L = loaded_rows(N)
    keep = np.ones(L, np.uint8)
    if c["keep"] == "holes":
        keep[[4, 8, 9]] = 0
        keep[[j for j in range(10, L - 1) if j % 3 == 1]] = 0
    elif c["keep"] == "one":
        keep[:] = 0
        keep[7 if c["corr"] == "firth" else 3] = 1
    K = int(keep.sum())
    q = max(1, K // 4)
    band = {"full": (0, K), "inner": (q, K - q) if K >= 3 else (0, K), "empty": (K // 2, K // 2)}[c["band"]]
    return dict(case=c, index=i, corr=c["corr"], N=N, T=T, Pc=Pc, L=L, keep=keep, K=K, band=band, eng=c["eng"],
                slots=None if i in NO_FORCE else c["slots"], cutoff=CUTOFF[(c["corr"], c["cut"])])


def case_id(i):
    c = CASES[i]
    s = "-".join(f"{k}{v}" if k in ("N", "slots") else str(v) for k, v in c.items())
    return f"{i}-{s}" + ("-dropped" if i in NO_FORCE and c["slots"] is not None else "")


_CACHE = {}


def build(i):
    """resolve(i) with the data: G [L][N] int8 (the loaded rows), Y, C, inc, nulls (test_gpu_assoc_spa.rebuild: mu, Z, kappa per trait)"""
    import test_gpu_assoc_firth as tf
    import test_gpu_assoc_spa as ts
    inp = resolve(i)
    key = (inp["corr"], inp["N"], inp["T"], inp["Pc"])
    if key not in _CACHE:
        if inp["corr"] == "firth":
            G, Y, Cm, inc, special, nulls = tf.inputs(*key[1:])
        else:
            G, Y, Cm, inc, special = ts.inputs(*key[1:])
            nulls = ts.rebuild(Y, Cm, inc)
        pick = list(range(inp["L"] - 1)) + [ALL_MISSING]
        _CACHE[key] = (np.ascontiguousarray(G[pick]), Y, Cm, inc, special, nulls)
    inp["G"], inp["Y"], inp["C"], inp["inc"], inp["special"], inp["nulls"] = _CACHE[key]
    inp["kept"] = np.flatnonzero(inp["keep"])
    return inp


def restated(inp):
    """the kept rows on the CPU alone: a dict with ua, flipped and z from test_gpu_assoc_score.restate / finish in f64, shaped like a
    device result, so that the device modules' item_inputs can be fed with it"""
    import test_gpu_assoc_score as sc
    Gk = inp["G"][inp["kept"]]
    mu = np.stack([n[0] for n in inp["nulls"]], 1)
    Bs, kappas = sc.panel(inp["Y"], inp["C"], inp["inc"], mu)
    ref = sc.restate(Gk, Bs, kappas, inp["inc"], inp["Pc"])
    fin = sc.finish(ref["ua"], ref["nobs"], ref["s1"], ref["s2"])
    return dict(ua=ref["ua"], flipped=fin["flipped"], z=fin["z"])


def listed(inp, r, margin=0.0):
    """the items the flag kernels list for a result r: z finite, |z| >= the cutoff (times 1 + margin), and for spa U != 0"""
    z = r["z"]
    with np.errstate(invalid="ignore"):
        m = np.isfinite(z) & (np.abs(z) >= inp["cutoff"] * (1.0 + margin))
    if inp["corr"] == "spa":
        m &= r["ua"][:, :, 0] != 0.0
    return m
