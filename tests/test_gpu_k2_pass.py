"""K2, Y = A^T T, of every kernel that computes it, held per element to a bar derived from its arithmetic -- through gpca_transform.

THE OBSERVABLE.  gpca_transform after a fit is one K2 pass and nothing else of weight (gpca_rsvd.cpp): launch_expand_loadings scatters the
f32 loadings U into T, launch_scale_rows makes T' = r o U and the 64-row partials of c = b^T U, stage_sum_c folds them, stage_AtT_local
quantises T', runs K2 and folds its partial tiles, and a right-multiplication by a 0 / 1 selection matrix (products by 1, sums with +0:
exact) keeps the k columns asked for.  U is what gpca_get_loadings returns, bit for bit; mu, sigma and keep are the test's own through
gpca_set_standardization.  So every input of the pass is known on the CPU and nothing corrects an error of the pass afterwards.  Whatever
the fit produced is the model's W; nothing else is read from the device and trusted.

THE EXACT MODES (int8 rows with 4 digit planes, 2-bit rows with 3 and with 4).  The model and both bars are test_gpu_exact_pass.py's,
imported: ``exact_pass_model`` (no missing call here), ``bounds``, ``check_against_bars``.  What this module adds is the input family
``zero_mu``: mu = 0 makes b = -0 r zero, and with it Tb, c and the u32 * 64 * sum |Tb| term of the bar against the model, which then is
    u64 (P + 2) |scale Yint|  +  the counted ties                          (u64 = 2^-53, P = ceil(Mpad / 64), scale = colmax / S)
and sigma from {1, 1/2, .., 1/32} makes r and Ta = r U exact in f32.  One unit of Yint is colmax / S = 7.6e-9 colmax (4 planes) or
1.2e-7 colmax (3 planes).  Every zero_mu case asserts, on the CPU, that a tie-free column exists and that its bar is below a QUARTER of
that unit at every sample: a single wrong integer anywhere in a K2 tile shows.  ``small_mu`` (mu uniform in 0.002 .. 0.02, sigma
log-uniform on [1/32, 1]) exercises c, launch_scale_rows' cpart and stage_sum_c; its bar carries the f32 term and the bar against
ref_project the ``generic`` roundings.  few_ties (at least 95 % of the columns tie-free) is asserted before any comparison.

GPCA_PREC_F32_MFMA (gemm_f32.hip, k_reduce_y; int8 and 2-bit rows, l <= 64).  gtt_plan (restated below) cuts Mpad into W row chunks of
rows_per_wave rows.  Within a chunk every (sample, column) is ONE f32 accumulator fed in row order by mfma_f32_32x32x2f32; a dosage is
decoded as an fp8 subnormal g 2^-9, so a product g T' is exact up to that power of two, and only the additions round: a chain of R
additions is off by at most ((1 + u32)^R - 1) sum |g Ta| <= u32 (R + 1) sum |g Ta| while R^2 u32 <= 2 (asserted; R <= 4224 here).
k_reduce_y adds the W partials in f64 (W additions), multiplies by 2^9 (exact) and adds c (one more).  Against the f64 truth built from
the same f32 Ta (``f32_pass_model``) the bar is therefore
    sum over the chunks of  u32 (rows of the chunk + 1) sum_{i in chunk} |g_in Ta_ij|
    + u64 (W + 1) (sum_i |g_in Ta_ij| + |c_j|)                 the fold
    + u64 (M + 1) sum_i |g_in Ta_ij|                           the truth's own f64 dot product
    + the c terms of ``bounds``:  u64 (P + 2) (|c_j| + sum_i |Tb_ij|) + u32 64 sum_i |Tb_ij|.
The chain term is a worst case: it catches misplaced or missing rows, chunks and tiles, not a last-bit defect.  Every factor is a unit
roundoff, a count read from the code or a formula over the inputs.

INPUTS.  Dosages 0 / 1 / 2 without a missing call, allele frequencies log-uniform on [0.05, 0.5] (row M - 1 at 0.5), seeded per shape.
keep drops every 7th row (3, 10, ..) and, at 4097 rows, all of rows 3968 .. 4095: the last full 128-row stage then holds only zero rows of
T', while row 4096, alone in its stage, stays.  After gpca_set_standardization the fit is gpca_rsvd(k, oversample, 1, seed).
gpca_rsvd refuses fewer than 2 samples, so K2 at N = 1 cannot be reached through a fit: the N = 1 case asserts that refusal and N = 2
(k = 2) stands in as the smallest sample count.

THE PLANS (``k2_plan``, ``f32_plan``: plan_math.h's gtt8_plan, gtt8_plan_batched, gtt8_plan_narrow and gtt_plan restated, with
gpca_rsvd.cpp's choice between them) say which branch a shape reaches.  test_restated_plans_reach_the_branches_the_shapes_are_chosen_for
(CPU) asserts the facts the shapes were chosen for, so a planner change that moves a shape off its branch turns that test red.

TEETH (CPU, unmarked).  On the device tests' own genotypes, standardisations and restated plans -- the loadings come from an f64
randomized PCA on the CPU -- the unmutated model sits inside every bar and each mutant leaves it: the short last row chunk left out; row
4096 (the neighbour of the all-zero stage) left out; one n-group's tile taken from the n-group before it; a chained workgroup's second
task written to the first task's slice of Ypart; one unit added to one element of Yint (required under zero_mu, recorded under small_mu);
the six of test_gpu_exact_pass.MUTATIONS; for f32 the last pair of 16-row groups of a chunk left out, the second column tile fed the
first tile's T', one chunk's partial counted twice in the fold.  Two of the six need what a transform's input does not have:
``missing_as_3`` runs on a copy with a few planted missing calls, and ``last_group_out_of_c`` is required under small_mu only (under
zero_mu c is identically zero and the mutant must equal the model).

Streamed handles accept gpca_set_standardization (it runs the stats pass over the panels first), so the streamed cases use both families.

Not reached, and why: K2 inside the fused streamed power sweep (launch_accum_y_scaled / launch_finish_y_sum, stage_power_fused) and the
sketch pass fed by launch_omega_planes are not reachable from gpca_transform; they are held the same way through two test hooks of their
own, in test_gpu_fused_sweep.py (gpca_device_power) and test_gpu_sketch_pass.py (gpca_device_sketch).  A fault common to every kernel
AND the model (a wrong reading of DESIGN.md) is out of reach by construction.  On GPCA_PREC_F32_MFMA only gross defects show (see above).
K2 at one sample is refused by gpca_rsvd.

Measured on one MI355X, the largest fraction of a bar over every case, sample and column (records, not thresholds; each test prints its
own with -s):
    against the model, zero_mu:   int8 0.45, 2-bit (3 planes) 0.49, 2-bit (4 planes) 0.45 -- the bar there is u64 (P + 2) |Y|, a few f64 roundings wide
    against the model, small_mu:  int8 0.024, 2-bit (3 planes) 0.028, 2-bit (4 planes) 0.024
    against ref_project:          zero_mu 0.89 / 0.90 / 0.89 (the quantisation bound alone, largest at about 30 rows), small_mu 0.38 / 0.68 / 0.38
    GPCA_PREC_F32_MFMA:           0.13 (zero_mu and small_mu, int8 and 2-bit rows; the chain term is a worst case)
The module's wall time there: 24 s for its 277 device cases; the 17 CPU cases (plans, teeth) take 27 s.
One value-only defect compiled into gtt_tiles_out of gemm_i8.hip on a scratch copy (+ 1 on ONE integer of the first tile of row chunk 1; k_gtt_d
and k_gtt_p store through it), run once: all 76 zero_mu cases whose plan has a second row chunk on those kernels went red (1e6 .. 4e7 times
the bar); the small_mu cases of the two-shard test (the only ones that run when the zero_mu half of a case has failed), every case with one
row chunk and every case on the narrow and the register-only kernels stayed green, and so did test_transform_after_a_fit and
test_rsvd_parity_i8 on the same library."""
import threading

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from test_gpu_exact_pass import (MISSING, MUTATIONS, U32, U64, bounds, check_against_bars, exact_pass_model, few_ties, int_dot,
                                 quantize, ref_project, scale_f32)

# mode -> (precision, storage, digit_planes argument, planes in use (0: f32), packed rows)
MODES = {"int8": (_lib.PREC_I8_EXACT, _lib.STORE_INT8, 0, 4, False), "2bit": (_lib.PREC_I8_EXACT, _lib.STORE_2BIT, 0, 3, True),
         "2bit4": (_lib.PREC_I8_EXACT, _lib.STORE_2BIT, 4, 4, True), "f32": (_lib.PREC_F32_MFMA, _lib.STORE_INT8, 0, 0, False),
         "f32_2bit": (_lib.PREC_F32_MFMA, _lib.STORE_2BIT, 0, 0, True)}
EXACT = ["int8", "2bit", "2bit4"]
FAMILIES = ["zero_mu", "small_mu"]
RECORD = {}                      # (mode, family) -> the largest fraction of the bar against the model seen so far


def round_up(a, b):
    return (a + b - 1) // b * b


# ---- the planners of plan_math.h, restated ---------------------------------------------------------------------------------------------------
def gtt_plan(Mpad, Npad, target):
    nb = Npad // 256
    W = min(max(target // nb, 1), Mpad // 32)
    rpw = round_up(-(-Mpad // W), 32)
    W = -(-Mpad // rpw)
    return dict(kind="f32", nblocks_n=nb, ngroups=(nb + 3) // 4, W=W, rows_per_wave=rpw, grid=(nb + 3) // 4 * W, group_samples=1024)


def gtt8_plan(Mpad, Npad, target):
    nb = Npad // 128
    W = max(target // nb, 1, (Mpad + (1 << 22) - 1) >> 22)
    W = min(W, Mpad // 128)
    rpw = round_up(-(-Mpad // W), 128)
    W = -(-Mpad // rpw)
    ng = (nb + 3) // 4
    return dict(kind="simple", nblocks_n=nb, ngroups=ng, W=W, rows_per_wave=rpw, grid=ng * W, tasks_per_wg=1, group_samples=512)


def gtt8_plan_batched(Mpad, Npad, target):
    nb = Npad // 128
    ng, S = (nb + 3) // 4, Mpad // 128
    grid0 = max(target // 8, 1)
    wmin, wmax = max(1, (S + 32767) // 32768), min(S, 1024)
    best, bestW = 1e300, wmin
    for W in range(wmin, max(wmin, wmax) + 1):
        T = W * ng
        k = (T + grid0 - 1) // grid0
        f = float(k * grid0) / float(T)
        f *= 1.0 + 3.0 * float(W) / float(S)
        f += float(W) * 256.0 / float(Mpad)
        if float(S) / float(W) * 16384.0 > 3.0 * 1048576.0:
            f += 0.02
        if f < best - 1e-12:
            best, bestW = f, W
    C = (S + bestW - 1) // bestW
    W = (S + C - 1) // C
    T = W * ng
    tpw = (T + grid0 - 1) // grid0
    return dict(kind="batched", nblocks_n=nb, ngroups=ng, S=S, C=C, W=W, rows_per_wave=C * 128, tasks_per_wg=tpw, grid=(T + tpw - 1) // tpw,
                group_samples=512)


def gtt8_plan_narrow(Mpad, N, target):
    nb = (N + 127) // 128
    W = min(max(target // nb, 1), Mpad // 128)
    rpw = round_up(-(-Mpad // W), 128)
    W = -(-Mpad // rpw)
    return dict(kind="narrow", nblocks_n=nb, ngroups=nb, W=W, rows_per_wave=rpw, grid=(W * nb + 3) // 4, tasks_per_wg=1, group_samples=128)


def waves_target(gtt_waves):
    return max(4, gtt_waves) if gtt_waves else 2048            # (gpca_create: gpca_config.reserved[2], 0 = the tuned default)


def k2_plan(M, N, packed, gtt_waves=0, flags=0):
    """the plan of an exact-path K2 launch over a resident matrix, as k2_plan of gpca_rsvd.cpp chooses it"""
    Mpad, Npad, target = round_up(M, 128), round_up(N, 1024 if packed else 256), waves_target(gtt_waves)
    if not packed and N <= 256 and not flags & _lib.CFG_NO_NARROW:
        return gtt8_plan_narrow(Mpad, N, min(target, 1024))
    return gtt8_plan(Mpad, Npad, target) if flags & _lib.CFG_SIMPLE_KERNELS else gtt8_plan_batched(Mpad, Npad, target)


def f32_plan(M, N, packed, gtt_waves=0):
    return gtt_plan(round_up(M, 128), round_up(N, 1024 if packed else 256), waves_target(gtt_waves))


def row_chunks(plan, M):
    """[(first row, end row)] of the plan's W row chunks over the padded rows (the last may be shorter)"""
    Mpad, rpw = round_up(M, 128), plan["rows_per_wave"]
    ch = [(w * rpw, min(Mpad, (w + 1) * rpw)) for w in range(plan["W"])]
    assert ch[-1][1] == Mpad and all(a < b for a, b in ch)
    return ch


def workgroup_tasks(plan, v):
    """the (row chunk, n-group) tasks of virtual workgroup v of a batched launch (K2Walk, gemm_i8.hip: v, v + grid, ..; n-group fastest)"""
    T = plan["W"] * plan["ngroups"]
    return [divmod(t, plan["ngroups"]) for t in range(v, min(T, v + plan["tasks_per_wg"] * plan["grid"]), plan["grid"])]


def test_restated_plans_reach_the_branches_the_shapes_are_chosen_for():
    M = 4097
    # narrow (int8 rows, N <= 256): one wave per (row chunk, 128-sample block), four per workgroup
    for N, tasks, grid, live_last in ((1, 33, 9, 1), (2, 33, 9, 1), (128, 33, 9, 1), (129, 66, 17, 2), (255, 66, 17, 2), (256, 66, 17, 2)):
        p = k2_plan(M, N, False)
        assert p["kind"] == "narrow" and p["W"] == 33 and p["W"] * p["nblocks_n"] == tasks and p["grid"] == grid and tasks - 4 * (grid - 1) == live_last
    assert k2_plan(M, 257, False)["kind"] == "batched" and k2_plan(M, 256, False, flags=_lib.CFG_NO_NARROW)["kind"] == "batched"
    assert k2_plan(M, 256, False, flags=_lib.CFG_NO_NARROW | _lib.CFG_SIMPLE_KERNELS)["kind"] == "simple" and k2_plan(M, 255, True)["kind"] == "batched"
    for N in (513, 1025):                                      # the last 512-sample n-group holds two 128-sample blocks of four
        p = k2_plan(M, N, False)
        assert p["nblocks_n"] % 4 == 2 and p["ngroups"] == p["nblocks_n"] // 4 + 1
    p = k2_plan(M, 1025, False)                                # every task one stage, shorter than the DMA prologue
    assert (p["S"], p["W"], p["C"]) == (33, 33, 1)
    p = k2_plan(M, 1025, True)
    assert (p["W"], p["C"]) == (17, 2) and row_chunks(p, M)[-1] == (4096, 4224)
    # chained tasks and short chunks
    p = k2_plan(M, 1025, False, 16)
    assert (p["W"], p["C"], p["tasks_per_wg"], p["grid"]) == (2, 17, 3, 2) and p["W"] * p["ngroups"] == 6 and row_chunks(p, M)[-1] == (17 * 128, 33 * 128)
    p = k2_plan(M, 1025, True, 24)
    assert (p["W"], p["C"], p["tasks_per_wg"], p["grid"]) == (2, 17, 3, 3) and p["W"] * p["ngroups"] == 8
    assert [w for w, _ in workgroup_tasks(p, 1)] == [0, 1, 1] and len(workgroup_tasks(p, 2)) == 2       # (a crossing; a dead last task)
    p = k2_plan(M, 2049, False, 24)
    assert (p["W"], p["tasks_per_wg"], p["grid"]) == (1, 2, 3) and p["W"] * p["ngroups"] == 5 and len(workgroup_tasks(p, 2)) == 1
    p = k2_plan(M, 2049, False, 64)
    assert (p["W"], p["C"], p["tasks_per_wg"], p["grid"]) == (3, 11, 2, 8) and p["W"] * p["ngroups"] == 15
    assert any(len({w for w, _ in workgroup_tasks(p, v)}) == 2 for v in range(8))
    for N in (1025, 2561):
        for packed in (False, True):
            p = k2_plan(M, N, packed, 4)
            assert p["grid"] == 1 and 3 <= p["tasks_per_wg"] <= 6 and len(workgroup_tasks(p, 0)) == p["W"] * p["ngroups"]
    p = k2_plan(M, 1025, False, 64, _lib.CFG_SIMPLE_KERNELS)
    assert (p["W"], p["rows_per_wave"]) == (6, 768) and row_chunks(p, M)[-1] == (3840, 4224)
    p = k2_plan(M, 1025, True, 64, _lib.CFG_SIMPLE_KERNELS)
    assert (p["W"], p["rows_per_wave"]) == (4, 1152) and row_chunks(p, M)[-1] == (3456, 4224)
    p = f32_plan(M, 1025, False, 64)
    assert (p["W"], p["rows_per_wave"]) == (12, 352)
    p = f32_plan(1790, 1025, False, 64)
    assert (p["W"], p["rows_per_wave"]) == (12, 160) and row_chunks(p, 1790)[-1] == (1760, 1792)
    for Mx, N in ((4097, 2049), (4097, 1), (31, 255)):         # the longest chain of the module's shapes keeps the bar's expansion valid
        for packed in (False, True):
            assert f32_plan(Mx, N, packed)["rows_per_wave"] ** 2 * U32 <= 2


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
_G, _STD = {}, {}


def genotypes(M, N):
    if (M, N) not in _G:
        rng = np.random.default_rng(1000 * N + M)
        p = np.exp(rng.uniform(np.log(0.05), np.log(0.5), size=(M, 1)))
        p[M - 1] = 0.5
        _G[(M, N)] = (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)
    return _G[(M, N)]


def keep_mask(M):
    keep = np.ones(M, np.uint8)
    keep[3::7] = 0
    if M == 4097:
        keep[3968:4096] = 0
    return keep


def standardisation(family, M, seed=0):
    """(mu, sigma, keep) of a family; seeded per row count (and per retry of a case whose quantisation ties)"""
    key = (family, M, seed)
    if key not in _STD:
        rng = np.random.default_rng([M, seed, FAMILIES.index(family)])
        if family == "zero_mu":
            mu, sigma = np.zeros(M, np.float32), (2.0 ** -rng.integers(0, 6, M)).astype(np.float32)
        else:
            mu, sigma = rng.uniform(0.002, 0.02, M).astype(np.float32), np.exp(rng.uniform(np.log(1 / 32), 0.0, M)).astype(np.float32)
        _STD[key] = (mu, sigma, keep_mask(M))
    return _STD[key]


def small_sketch(M, N):
    """(k, oversample) of the rows x samples grid: (22, 10) where the kept rows and the samples allow it, else (5, 0) (N = 2: (2, 0))"""
    n = min(int(keep_mask(M).sum()), N)
    return (22, 10) if n >= 32 else ((5, 0) if n >= 5 else (n, 0))


def cpu_loadings(G, mu, sigma, keep, k):
    """f32 loadings [M][k] of an f64 randomized PCA (one power iteration) on the kept rows: the W of the CPU teeth"""
    rows = np.flatnonzero(keep)
    A = (G[rows].astype(np.float64) - mu[rows].astype(np.float64)[:, None]) / sigma[rows].astype(np.float64)[:, None]
    Q, _ = np.linalg.qr(A.T @ np.random.default_rng(k).standard_normal((len(rows), k)))
    U, _, _ = np.linalg.svd(A @ Q, full_matrices=False)
    W = np.zeros((G.shape[0], k), np.float32)
    W[rows] = U.astype(np.float32)
    return W


# ---- the f32 path: truth, bar, simulator ---------------------------------------------------------------------------------------------------
def c_terms(Tb, M):
    """the c terms of ``bounds`` [k] (what remains of its bar against the model when both integer sides are empty)"""
    k = Tb.shape[1]
    z, zi = np.zeros(k), np.zeros((1, k))
    c = np.sum(Tb.astype(np.longdouble), axis=0).astype(np.float64)
    m = dict(Tb=Tb, M=M, sa=z, sb=z, Yia=zi, Yib=zi, c=c, ties_a=z, ties_b=z, ga=np.zeros((1, 1)), miss=np.zeros((1, 1)), Ta=Tb)
    return c, bounds(m, False)[0][0]


def f32_pass_model(G, mu, sigma, W, plan):
    """(truth [N][k] in f64 from the f32 Ta and Tb, bar [N][k]) of one GPCA_PREC_F32_MFMA pass: the module docstring's formulas"""
    M = G.shape[0]
    _, _, _, Ta, Tb = scale_f32(mu, sigma, W)
    g, ta = G.astype(np.float64), Ta.astype(np.float64)
    assert not np.any(G == MISSING)
    c, cbar = c_terms(Tb, M)
    truth = g.T @ ta + c[None, :]
    chain, absall = np.zeros_like(truth), np.zeros_like(truth)
    for r0, r1 in row_chunks(plan, M):
        assert (r1 - r0) ** 2 * U32 <= 2
        a = g[r0:r1].T @ np.abs(ta[r0:r1])
        chain += U32 * (r1 - r0 + 1) * a
        absall += a
    bar = chain + U64 * (plan["W"] + 1) * (absall + np.abs(c)[None, :]) + U64 * (M + 1) * absall + cbar[None, :]
    return truth, bar


def simulate_k2_f32(G, mu, sigma, W, plan, mutate=None):
    """Y [N][k] as k_gtt_f32 and k_reduce_y make it: per row chunk one f32 accumulator per element walking the rows in order (g T' is exact, every
    addition rounds once), the chunks summed in f64, c added.  Mutants: the last 32 rows of chunk 0 left out; columns 32 .. of T' taken
    from columns 0 ..; chunk 0 counted twice."""
    M, N = G.shape
    _, _, _, Ta, Tb = scale_f32(mu, sigma, W)
    if mutate == "second_tile_first_t":
        assert Ta.shape[1] > 32
        Ta = Ta.copy(); Ta[:, 32:] = Ta[:, :Ta.shape[1] - 32]
    g = G.astype(np.float32)
    parts = []
    for r0, r1 in row_chunks(plan, M):
        hi = r1 - 32 if mutate == "last_group_pair_out" and r0 == 0 else r1
        acc = np.zeros((N, Ta.shape[1]), np.float32)
        for i in range(r0, min(hi, M)):
            if np.any(Ta[i] != 0):
                acc += g[i][:, None] * Ta[i][None, :]
        parts.append(acc.astype(np.float64))
    if mutate == "chunk_counted_twice":
        parts.append(parts[0])
    s = np.zeros_like(parts[0])
    for p in parts:
        s += p
    return s + np.sum(Tb.astype(np.float64), axis=0)[None, :]


def fraction(d, bar):
    return float(np.max(np.where(bar > 0, d / np.where(bar > 0, bar, 1), np.where(d > 0, np.inf, 0)), initial=0))


def check_f32(tr, G, mu, sigma, W, plan, what):
    truth, bar = f32_pass_model(G, mu, sigma, W, plan)
    assert tr.shape == truth.shape and np.all(np.isfinite(tr)), what
    f = fraction(np.abs(tr - truth), bar)
    print(f"{what}: max |Y_device - Y_truth| / bar = {f:.3g}")
    assert np.all(np.abs(tr - truth) <= bar), f"{what}: {f:.3g} of the bar"
    return f


# ---- the exact path: what the zero_mu family is for ------------------------------------------------------------------------------------------
def assert_one_unit_is_visible(m, nd, what):
    """a tie-free column exists, and its bar against the model is below a quarter of one unit of Yint at every sample"""
    free = np.flatnonzero((m["ties_a"] == 0) & (m["ties_b"] == 0) & (m["sa"] > 0))
    assert len(free) > 0, what + ": no tie-free column"
    bar, _ = bounds(m, False)
    worst = float(np.max(bar[:, free] / m["sa"][None, free]))
    assert worst < 0.25, f"{what}: the bar is {worst:.3g} units of Yint wide"
    return free


def recombine(m, Yia):
    """Y of the model from (possibly mutated) integer sums: exact_pass_model's last step without missing calls"""
    ld = np.longdouble
    return (m["sa"].astype(ld)[None, :] * Yia.astype(ld) + m["c"].astype(ld)[None, :]).astype(np.float64)


PLAN_MUTANTS = ["short_last_chunk_out", "row_after_the_zero_stage_out", "ngroup_from_the_one_before", "second_task_to_first_slice", "one_unit"]


def planned_yint(m, nd, plan, mutate=None, col=0):
    """Yint_a [N][k] built as K2 builds it -- one partial tile per (row chunk, n-group), then the fold -- with one of PLAN_MUTANTS"""
    M = m["M"]
    N = m["ga"].shape[1]
    qa = quantize(m["Ta"], nd)[0]
    ga = m["ga"].astype(np.int64)
    if mutate == "row_after_the_zero_stage_out":
        ga = ga.copy(); ga[M - 1] = 0
    parts = [int_dot(ga[r0:min(r1, M)], qa[r0:min(r1, M)]) for r0, r1 in row_chunks(plan, M)]
    gs = plan["group_samples"]
    if mutate == "short_last_chunk_out":
        parts[-1][:] = 0
    if mutate == "ngroup_from_the_one_before":
        n = min(gs, N - gs)
        assert n > 0
        parts[0][gs:gs + n] = parts[0][:n]
    if mutate == "second_task_to_first_slice":
        (w1, g1), (w2, g2) = workgroup_tasks(plan, 0)[:2]
        tile = np.zeros((gs, parts[0].shape[1]), np.int64)
        src = parts[w2][g2 * gs:(g2 + 1) * gs].copy()
        tile[:len(src)] = src
        parts[w2][g2 * gs:(g2 + 1) * gs] = 0
        dst = parts[w1][g1 * gs:(g1 + 1) * gs]
        dst[:] = tile[:len(dst)]
    Y = sum(parts)
    if mutate == "one_unit":
        Y = Y.copy(); Y[N // 2, col] += 1
    return Y


# ---- teeth (CPU) ------------------------------------------------------------------------------------------------------------------------------
# (N, packed rows, gtt_waves, simple kernels): the plans of the chained cases and the default ones
TEETH_PLANS = [(1025, False, 0, 0), (1025, True, 0, 0), (1025, False, 16, 0), (1025, True, 24, 0), (2049, False, 64, 0), (1025, False, 64, 1)]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("nd", [3, 4])
def test_the_bar_rejects_every_plan_mutant(nd, family):
    M, k = 4097, 30
    for N, packed, gtt_waves, simple in TEETH_PLANS:
        if (nd == 3) != packed and not (nd == 4 and packed and gtt_waves == 0):      # (3 planes: packed rows only; 4 planes: both)
            continue
        G = genotypes(M, N)
        mu, sigma, keep = standardisation(family, M)
        W = cpu_loadings(G, mu, sigma, keep, k)
        m = exact_pass_model(G, mu, sigma, W, nd)
        assert m["digits_ok"] and few_ties(m)
        bar, _ = bounds(m, family == "small_mu")
        col = int(assert_one_unit_is_visible(m, nd, "teeth")[0]) if family == "zero_mu" else int(np.argmax(m["sa"] > 0))
        plan = k2_plan(M, N, packed, gtt_waves, _lib.CFG_SIMPLE_KERNELS if simple else 0)
        assert np.array_equal(planned_yint(m, nd, plan), m["Yia"]) and np.array_equal(recombine(m, m["Yia"]), m["Y"])
        for mut in PLAN_MUTANTS:
            if mut == "second_task_to_first_slice" and plan["tasks_per_wg"] < 2:
                continue
            if mut == "short_last_chunk_out" and plan["W"] < 2:
                continue
            d = np.abs(recombine(m, planned_yint(m, nd, plan, mut, col)) - m["Y"])
            f = fraction(d, bar)
            print(f"nd={nd} {family} N={N} packed={packed} gtt_waves={gtt_waves} simple={simple}: mutant {mut}: max |dY| / bar = {f:.3g}")
            if mut == "one_unit" and family == "small_mu":
                continue                                       # (recorded: the f32 term of c may hide one unit there)
            assert np.any(d > bar), f"the bar lets the mutant '{mut}' through ({f:.3g} of it)"


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("M", [33, 4097])
@pytest.mark.parametrize("nd", [3, 4])
def test_the_bar_rejects_the_six_of_the_exact_pass(nd, M, family):
    N = 1025
    k = 30 if M == 4097 else 5
    G = genotypes(M, N)
    mu, sigma, keep = standardisation(family, M)
    W = cpu_loadings(G, mu, sigma, keep, k)
    # (colmax_first_half wraps a digit only where the second half of the rows holds a maximum more than twice the first half's: column k - 1
    #  gets one in the last row, four times the rest, as make_inputs of the exact-pass module plants it)
    W[M - 1, k - 1] = np.float32(4 * np.max(np.abs(W[:, k - 1]) / sigma) * sigma[M - 1])
    Gm = G.copy()                                              # (a transform's input has no missing call: missing_as_3 gets a copy with a few)
    rng = np.random.default_rng(M + nd)
    Gm[rng.choice(np.flatnonzero(keep), 8), rng.integers(0, N, 8)] = MISSING
    for mut in MUTATIONS:
        Gx = Gm if mut == "missing_as_3" else G
        m = exact_pass_model(Gx, mu, sigma, W, nd)
        assert m["digits_ok"] and few_ties(m)
        bar, _ = bounds(m, family == "small_mu")
        d = np.abs(exact_pass_model(Gx, mu, sigma, W, nd, mutate=mut)["Y"] - m["Y"])
        print(f"nd={nd} M={M} {family}: mutant {mut}: max |dY| / bar = {fraction(d, bar):.3g}")
        if mut == "last_group_out_of_c" and family == "zero_mu":
            assert np.all(d == 0)                              # (c is identically zero: nothing to leave out)
        else:
            assert np.any(d > bar), f"the bar lets the mutant '{mut}' through"


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("M", [1790, 4097])
def test_the_f32_bar_rejects_its_mutants(M, family):
    N, k = 1025, 33
    G = genotypes(M, N)
    mu, sigma, keep = standardisation(family, M)
    W = cpu_loadings(G, mu, sigma, keep, k)
    for gtt_waves in (64, 0):
        plan = f32_plan(M, N, False, gtt_waves)
        truth, bar = f32_pass_model(G, mu, sigma, W, plan)
        for mut in (None, "last_group_pair_out", "second_tile_first_t", "chunk_counted_twice"):
            d = np.abs(simulate_k2_f32(G, mu, sigma, W, plan, mut) - truth)
            f = fraction(d, bar)
            print(f"f32 M={M} {family} gtt_waves={gtt_waves}: mutant {mut}: max |dY| / bar = {f:.3g}")
            assert f <= 1 if mut is None else np.any(d > bar), f"{mut}: {f:.3g} of the bar"


# ---- the device ------------------------------------------------------------------------------------------------------------------------------
def open_engine(mode, **kw):
    prec, store, planes, _, _ = MODES[mode]
    return gpca.GpcaEngine(precision=prec, storage=store, digit_planes=planes, **kw)


def fit_and_transform(e, M, k, os_, mu, sigma, keep):
    """the fit, then (W [M][k] from the loadings, the transform)"""
    e.set_standardization(mu, sigma, keep)
    e.rsvd(k, os_, 1, seed=7)
    rows = e.pca_snp_rows()
    assert np.array_equal(rows, np.flatnonzero(keep))
    W = np.zeros((M, k), np.float32)
    W[rows] = e.loadings()
    return W, e.transform()


def record(mode, family, f):
    RECORD[(mode, family)] = max(RECORD.get((mode, family), 0.0), f)
    print(f"    largest fraction of the bar so far, {mode} {family}: {RECORD[(mode, family)]:.3g}")


def check_case(tr, G, mu, sigma, W, mode, family, plan, what):
    """one device result against its bars (exact modes: both bars of the exact pass; f32: the chain bar)"""
    nd = MODES[mode][3]
    assert tr.shape == (G.shape[1], W.shape[1]), what
    if nd:
        m = exact_pass_model(G, mu, sigma, W, nd)
        assert m["digits_ok"] and few_ties(m), what + ": the seeded input ties too often: change the seed"
        if family == "zero_mu":
            assert_one_unit_is_visible(m, nd, what)
        _, f, _ = check_against_bars(tr, G, mu, sigma, W, nd, family != "zero_mu", what)
    else:
        f = check_f32(tr, G, mu, sigma, W, plan, what)
    record(mode, family, f)
    return f


def run_case(mode, M, N, k, os_, families=FAMILIES, open_fn=None, **kw):
    G = genotypes(M, N)
    packed = MODES[mode][4]
    for family in families:
        mu, sigma, keep = standardisation(family, M)
        with open_engine(mode, **kw) as e:
            if open_fn is None:
                e.upload_genotypes_i8(G)
            else:
                open_fn(e, G)
            W, tr = fit_and_transform(e, M, k, os_, mu, sigma, keep)
        plan = f32_plan(M, N, packed, kw.get("gtt_waves", 0))
        check_case(tr, G, mu, sigma, W, mode, family, plan, f"transform {mode} {family} M={M} N={N} k={k}+{os_} {kw or ''}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 513, 1025, 2049])
@pytest.mark.parametrize("M", [31, 32, 33, 129, 4097])
def test_transform_rows_and_samples(mode, M, N):
    if N == 1:                                                 # gpca_rsvd refuses fewer than 2 samples: K2 at one sample is out of a fit's reach
        mu, sigma, keep = standardisation("zero_mu", M)
        with open_engine(mode) as e:
            e.upload_genotypes_i8(genotypes(M, 1))
            e.set_standardization(mu, sigma, keep)
            with pytest.raises(_lib.GpcaError) as ex:
                e.rsvd(1, 0, 1, seed=7)
        assert ex.value.status == _lib.GPCA_ERR_BAD_ARG
        return
    k, os_ = small_sketch(M, N)
    run_case(mode, M, N, k, os_)


# (N, storage, gtt_waves): test_restated_plans_.. says what each reaches
CHAINED = [(1025, "int8", 16), (1025, "2bit", 24), (2049, "int8", 24), (2049, "int8", 64), (1025, "int8", 4), (1025, "2bit", 4), (2561, "int8", 4),
           (2561, "2bit", 4), (1025, "int8", 64), (1025, "2bit", 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("simple", [0, 1])
@pytest.mark.parametrize("N,rows,gtt_waves", CHAINED)
def test_transform_chained_tasks_and_short_chunks(N, rows, gtt_waves, simple):
    """k_gtt_d / k_gtt_p with several chained tasks per workgroup, short last row chunks, dead last tasks, and the same shapes on the
    register-only kernels (GPCA_CFG_SIMPLE_KERNELS), whose gtt8_plan cuts the rows differently"""
    for mode in (["int8"] if rows == "int8" else ["2bit", "2bit4"]):
        run_case(mode, 4097, N, 30, 0, ["zero_mu"], gtt_waves=gtt_waves, flags=_lib.CFG_SIMPLE_KERNELS if simple else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("simple", [0, 1])
def test_transform_no_narrow(simple):
    """N = 256 on int8 rows through the wide kernels (GPCA_CFG_NO_NARROW)"""
    run_case("int8", 4097, 256, 30, 0, ["zero_mu"], flags=_lib.CFG_NO_NARROW | (_lib.CFG_SIMPLE_KERNELS if simple else 0))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32", "f32_2bit"])
@pytest.mark.parametrize("M", [1790, 4097])
def test_transform_f32_row_chunks(mode, M):
    """gtt_waves = 64: 12 row chunks of 352 rows at 4097 rows, of 160 at 1790 with a last chunk of 32 (int8 rows)"""
    run_case(mode, M, 1025, 30, 0, ["zero_mu"], gtt_waves=64)


WIDTHS = [(1, 0), (32, 0), (33, 0), (54, 10), (64, 0), (65, 0), (118, 10), (128, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode,k,os_", [(m, k, o) for m in MODES for k, o in WIDTHS if k + o <= 64 or m in EXACT])
def test_transform_sketch_widths(mode, k, os_):
    """one, two and four 32-column halves; all k columns of the transform are checked"""
    run_case(mode, 4097, 1025, k, os_, ["zero_mu"])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", EXACT)
@pytest.mark.parametrize("fused", [True, False])
def test_transform_streamed_panels(mode, fused):
    """panel_rows = 1024 does not divide 4097 (the last panel holds one row): the per-panel k2_plan, the Td offset row0 >> 5,
    launch_accum_y_i8 / launch_finish_y_i8"""
    def open_stream(e, G):
        e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), G.shape[0], G.shape[1], panel_rows=1024, ring_slots=2, fused=fused)
    run_case(mode, 4097, 1025, 30, 0, open_fn=open_stream)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("mode", list(MODES))
def test_transform_two_row_shards_one_gpu(mode, family):
    """two row shards on one GPU through the allreduce hook.  Each rank quantises with its own column maxima: the model is the sum of the two
    shards' models, the bar the sum of their bars plus u64 (|Y_0| + |Y_1|) for the one f64 addition of the exchange."""
    M, N, k = 4097, 1025, 30
    G = genotypes(M, N)
    mu, sigma, keep = standardisation(family, M)
    spans = [gpca.shard_rows(M, 2, r) for r in range(2)]
    barrier = threading.Barrier(2, timeout=120); bufs = [None, None]; res = [None, None]; errs = []

    def run(rank):
        try:
            a, b_ = spans[rank]
            with open_engine(mode) as e:
                e.upload_genotypes_i8(G[a:b_])
                e.set_standardization(mu[a:b_], sigma[a:b_], keep[a:b_])

                def hook(buf):
                    bufs[rank] = buf.copy(); barrier.wait()
                    buf[:] = bufs[0] + bufs[1]; barrier.wait()
                e.set_allreduce_hook(hook, 2, rank, a)
                e.rsvd(k, 0, 1, seed=7)
                W = np.zeros((b_ - a, k), np.float32)
                W[e.pca_snp_rows()] = e.loadings()
                res[rank] = (W, e.transform())
        except BaseException as ex:  # noqa: BLE001 -- reported by the main thread
            errs.append(ex); barrier.abort()
    ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    [t.start() for t in ts]; [t.join() for t in ts]
    assert not errs, errs
    assert np.array_equal(res[0][1], res[1][1])
    tr, nd, packed = res[0][1], MODES[mode][3], MODES[mode][4]
    model, bar, parts_abs = np.zeros((N, k)), np.zeros((N, k)), np.zeros((N, k))
    truth, bar_truth = np.zeros((N, k)), np.zeros((N, k))
    for rank, (a, b_) in enumerate(spans):
        Gs, Ws = G[a:b_], res[rank][0]
        if nd:
            m = exact_pass_model(Gs, mu[a:b_], sigma[a:b_], Ws, nd)
            assert m["digits_ok"] and few_ties(m)
            if family == "zero_mu":
                assert_one_unit_is_visible(m, nd, f"rank {rank}")
            bm, bt = bounds(m, family != "zero_mu")
            y = m["Y"]
            truth += ref_project(Gs, mu[a:b_], sigma[a:b_], Ws)[0]; bar_truth += bt
        else:
            y, bm = f32_pass_model(Gs, mu[a:b_], sigma[a:b_], Ws, f32_plan(b_ - a, N, packed))
        model += y; bar += bm; parts_abs += np.abs(y)
    bar += U64 * parts_abs
    what = f"two shards {mode} {family}"
    f = fraction(np.abs(tr - model), bar)
    print(f"{what}: max |Y_device - Y_model| / bar = {f:.3g}")
    assert np.all(np.isfinite(tr)) and np.all(np.abs(tr - model) <= bar), f"{what}: {f:.3g} of the bar"
    if nd:
        assert np.all(np.abs(tr - truth) <= bar_truth + U64 * parts_abs), what + ": against ref_project"
    record(mode, family, f)


@pytest.mark.gpu
def test_transform_compact_child():
    """keep at a fifth of 70 000 rows: gpca_rsvd and gpca_transform run on the gathered child, whose matrix is the kept rows in order"""
    M, N, k, mode, family = 70_000, 320, 30, "int8", "zero_mu"
    G = genotypes(M, N)
    rng = np.random.default_rng(0)
    keep = (rng.random(M) < 0.2).astype(np.uint8)
    mu, sigma = np.zeros(M, np.float32), (2.0 ** -rng.integers(0, 6, M)).astype(np.float32)
    rows = np.flatnonzero(keep)
    with open_engine(mode) as e:
        e.upload_genotypes_i8(G)
        e.set_standardization(mu, sigma, keep)
        e.enable_timings(True)
        e.rsvd(k, 0, 1, seed=7)
        assert np.array_equal(e.pca_snp_rows(), rows)
        Wc = e.loadings()
        e.reset_timings()
        tr = e.transform()
        tim = e.timings()
    assert abs(tim["gemm_GtT"]["bytes"] / tim["gemm_GtT"]["launches"] / N - len(rows)) < 1, "the transform did not run on the compact child"
    check_case(tr, G[rows], mu[rows], sigma[rows], Wc, mode, family, None, f"compact child {mode} {family}")
