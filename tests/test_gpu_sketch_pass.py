"""The sketch Y = A^T Omega, the first thing every gpca_rsvd call does, held per element to a bar derived from its arithmetic -- through
the test hook gpca_device_sketch (include/gpca.h), which runs the product's own stage functions (stage_sketch, stage_sum_c,
stage_AtT_local) and returns the rank-local dY before any exchange.  Style and helpers of test_gpu_k2_pass.py and test_gpu_exact_pass.py.

WHY A HOOK.  After the sketch only span(Y) survives into a result, multiplied by cond(Y); the fits of the parity tests run power
iterations over matrices with a spectral gap and converge to the same subspace whatever Omega was.  Through the hook every element of Y
is compared.  A per-column error that stays inside span(Y) (a column scaled, two columns exchanged) is visible here and cannot change any
product result; no end-to-end check is added for it.

THE MODEL (``sketch_model``; written from kernels.hip's k_omega, its Td branch, and oracle/gpca_oracle.c's omega4 -- never from device
outputs).  Rows used = the rows keep leaves with |sigma| >= 1e-9; r = 1 / sigma, b = -mu r in f32, 0 on every other row.
    z   = oracle.omega at the ORIGINAL index of each row used (+ snp_offset), Philox counter (index low, index high, column / 4), key = seed
    zf  = f32(z),   T = f32(r zf)  (one __fmul_rn),   bound = 6.67 f64(max r),   S = 0.49 * 128^4 (4 planes) or 0.49 * 256^3 (3 planes)
    v   = rint(f64(T) * (S / bound))  as an integer; its signed digits must fit the ranges the kernel header states (asserted)
    Yint = G^T v  exactly,   c_j = sum_i b_i zf_ij,   Y = (bound / S) Yint + c.
The column scale is the same for every column, shard, panel and child: rmax is the maximum over the rows USED (a dropped row's 1 / sigma
must not enter: r is 0 there).

THE BAR AGAINST THE MODEL is ``bounds``' of test_gpu_exact_pass.py with sa = bound / S and Tb = b o zf (its f32 term u32 64 sum |Tb| covers
the 64-row partial of c in either branch of k_omega: L = 32, two half-waves and one __shfl_xor; the generic column walk), plus two kinds
of counted ties:
    (1) an entry of f64(T) * inv within 4 ulp of a half-integer may round either way: count_j * bound / S -- unless the product
        T * 0.49 B^nd / (6.67 rmax), taken in rational arithmetic, IS a half-integer.  S / bound = (49 / 667) 2^e / rmax: where rmax is a
        power of two (zero_mu: always) every T whose 24-bit significand is a multiple of 667 in one binade is such an entry, 1e-4 of
        them, half the columns at 4097 rows and nearly all at 23 000.  Their f64 images sit on the half-integer or an ulp beside it,
        fixed by the two IEEE operations the kernel and the model share (S / bound; one multiplication, then __double2int_rn, half to
        even): they are no ties, the model's integer is required (the narrower bar), and the tie-free share below is asked of the rest;
    (2) an entry of z within 4 f64 ulps of an f32 rounding boundary (the device's omg_box_muller is within 2e-16 of libm, not bit-equal):
        each adds 2 u32 |g T| to its column's bar at every sample.
By arithmetic the share of the remaining tied entries is about 1e-7; at least 95 % of the columns are tie-free, asserted on the CPU
before any launch.
THE BAR AGAINST THE TRUTH (A^T oracle-Omega in f64, A = (g - mu) / sigma in f64) is ``bounds(.., generic = True)`` -- the quantisation
0.5 (bound / S) sum_i g plus the f32 roundings of r, b, T, Tb -- with the 2 of its u32 sum |g Ta| term raised to 3: z rounds to f32 too.
GPCA_PREC_F32_MFMA (launch_omega with the blocked Tb, l <= 64): ``f32_pass_model`` of test_gpu_k2_pass.py with W = zf, i.e. Ta = f32(r zf),
and its chain bar, plus the ties of kind (2).

FAMILIES.  ``zero_mu`` (mu = 0, sigma from {1, 1/2, .., 1/32}): c = 0, the model bar is u64 (P + 2) |Y|, and every case asserts that in
a tie-free column this is below a QUARTER of one integer unit bound / S at every sample: one wrong integer anywhere shows.  ``small_mu``
(test_gpu_k2_pass.py's) exercises c.

SHAPES (the smallest at which k_omega can go wrong).  M in {1, 63, 64, 65, 127, 128, 129, 4097} crossed with edge_keeps(M): the wave's
live = i < M edge, the pad rows M .. Mpad (zero planes, nothing in c), one row only.  The largest r (zero_mu: sigma = 1/16 beside a
dropped 1/32, the other rows 1 .. 1/8; small_mu: 1 / 19.3 beside a dropped 1 / 1930, the others in [1/16, 1]) sits on the first kept
row (every row, zero_mu), on the last (every row, small_mu; last block dropped; every seventh) and the largest 1 / sigma on a DROPPED
row (last block dropped, one row, every seventh).
l in {1, 31, 32, 33, 64, 65, 100, 128}: the three instantiations <33>, <65>, <129, 1> and partial quads (4 jq < l <= 4 jq + 3); columns
>= l must not contribute; N = 5 (narrow on int8 rows) and N = 300; l > N, and l > 64 on GPCA_PREC_F32_MFMA, assert the refusal.  Seeds 7
and 0x9E3779B97F4A7C15.  snp_offset 0, 5 and 2^32 - 40 at 129 rows (the rows straddle the word boundary of the Philox counter), set
through set_allreduce_hook(fn, 1, 0, offset); the hook must not be called.  The compact child: 70 000 x 300, a third of the rows kept
irregularly, l = 33, int8 and 2-bit rows: on_child = 1, again with GPCA_CFG_NO_COMPACT on_child = 0, both inside the same model with Omega
by original index.  A streamed handle of 4097 rows in panels of 2048 (the last holds one row), fused on and off: the same bits as each
other and as the resident handle, once with row 4096 kept and carrying the largest r (every seventh row dropped) and once with that
panel all-dropped (last block dropped).

END TO END (the span identity of test_gpu_eigensnp_stages.py's i2_bar, its count restated): after gpca_rsvd(l, 0, 0, seed) with Pn an
orthonormal basis of span(scores_f64),  |((I - Pn Pn^T) Y_model)_.j|_2 <= |bar_.j|_2 + count u64 |Y_.j|_2,
count = 2 l sqrt(l) cond(Y) + (l + 2) sqrt(l) + 2 N, after asserting cond(Y_true)^2 u64 < 1: the hook and the product run the same sketch.

TEETH (CPU, unmarked).  On the device cases' own inputs the unmutated model sits inside both bars and every mutant of ``MUTANTS`` leaves
the bar against the model: Omega zeroed on the rows of the last 64-row wave; Omega by local instead of original index (child case); the
high word of the index dropped (straddle case); the high word of the seed dropped; column l - 1 zeroed; the halves of a Box-Muller pair
swapped; rmax over all rows instead of the kept ones (another grid; under small_mu the dropped row's 1 / sigma is 100 times the kept
maximum, so that the coarser grid's quantisation noise clears the f32 term of c at 3 and at 4 planes); one unit added to one integer
(required under zero_mu, recorded under small_mu, where the f32 term of c may hide a few units); z left in f64 (likewise); the last
64-row group left out of c (small_mu only); the base-128 split used where nd = 3.

Measured on one MI355X, the largest fraction of a bar over every case, sample and column (records, not thresholds; each test prints its
own with -s):
    against the model, zero_mu:   int8 0.46, 2-bit (3 planes) 0.46, 2-bit (4 planes) 0.46 -- the bar there is u64 (P + 2) |Y|; every exact
                                  half-integer rounded as the model rounds it
    against the model, small_mu:  int8 0.026, 2-bit (3 planes) 0.026, 2-bit (4 planes) 0.026
    against the truth:            zero_mu 0.35 / 0.73 / 0.35, small_mu 0.42 / 0.65 / 0.42 (the quantisation bound, largest at one kept row)
    GPCA_PREC_F32_MFMA:           0.088 (int8 and 2-bit rows, both families; the chain term is a worst case)
    the span identity:            0.0023 (int8, l = 33, cond(Y) = 7.4), 0.00029 (2-bit, l = 100, cond(Y) = 19)
The module's wall time there: 6 s for its 139 device cases (the four compact-child cases 0.3 - 0.4 s each); the 9 CPU cases take 5 s.
Two value-only defects compiled into k_omega's Td branch on a scratch copy, each run once with this module, test_rsvd_parity_i8,
test_rsvd_i8_sketch_width_and_iteration_edges and test_transform_after_a_fit on the same library:
  * ONE unit added to ONE integer (row 64, column 0): 52 cases of this module went red -- every exact-mode case with a kept row 64 and a
    sample that carries it (all of rows_and_keep_masks from 65 rows on, widths at N = 300, both offsets, the streamed handles, the
    zero_mu compact child, both span identities); the GPCA_PREC_F32_MFMA cases, the shapes of at most 64 rows, N = 5 and the small_mu
    compact child stayed green, and so did all 17 cases of the three older tests.
  * the top digit plane of wave 1 (rows 64 .. 127) zero: 57 cases of this module red; of the older tests all 5 cases of
    test_rsvd_parity_i8 and all 6 of test_rsvd_i8_sketch_width_and_iteration_edges went red as well (a defect of this size moves a fit
    by more than 1e-4 on their data, power iterations or not), the 6 of test_transform_after_a_fit stayed green.
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from _edges import edge_keeps
from test_gpu_exact_pass import U32, U64, bounds, digit_scale, int_dot, split_digits
from test_gpu_k2_pass import MODES, EXACT, f32_pass_model, f32_plan, fraction, genotypes

from oracle import oracle

FAMILIES = ["zero_mu", "small_mu"]
SEEDS = [7, 0x9E3779B97F4A7C15]
RECORD = {}


# ---- Omega and the model ---------------------------------------------------------------------------------------------------------------------
def draw(rows, M, l, seed, offset, mutate=None):
    """z [len(rows)][l] in f64: the oracle's normals at the rows' original indices, or one of the mutants that change the draw"""
    l4 = (l + 3) // 4 * 4
    if mutate == "seed_high_dropped":
        assert seed >> 32
        seed &= 0xFFFFFFFF
    if mutate == "local_index":
        z = oracle.omega(len(rows), l4, seed, offset)
    elif mutate == "index_high_dropped":
        assert offset + M > 1 << 32 > offset
        wrapped, plain = oracle.omega(M, l4, seed, offset - (1 << 32))[rows], oracle.omega(M, l4, seed, offset)[rows]
        z = np.where(((rows + offset) >> 32 > 0)[:, None], wrapped, plain)
    else:
        z = oracle.omega(M, l4, seed, offset)[rows]
    if mutate == "pair_swapped":
        z = z[:, np.arange(l4) ^ 1]
    z = np.ascontiguousarray(z[:, :l])
    if mutate == "last_column_zero":
        z[:, l - 1] = 0
    if mutate == "last_wave_zero":
        z[rows >= (M - 1) // 64 * 64] = 0
    return z


def f32_boundary_ties(z):
    """entries of z (f64) within 4 f64 ulps of the midpoint of two neighbouring f32 values"""
    zf = z.astype(np.float32)
    tie = np.zeros(z.shape, bool)
    for to in (np.float32(np.inf), np.float32(-np.inf)):
        mid = 0.5 * (zf.astype(np.float64) + np.nextafter(zf, to).astype(np.float64))
        tie |= np.abs(z - mid) <= 4 * np.spacing(np.abs(z))
    return tie


def used_rows(mu, sigma, keep):
    r, b = oracle.scale_shift(mu, sigma, keep)
    return np.flatnonzero(r != 0), r, b


def sketch_model(G, mu, sigma, keep, l, seed, offset, nd, mutate=None, rows_run=None, col=0):
    """The fixed-point model of the exact sketch (module docstring).  rows_run: the row count of the matrix the device ran on (the compact
    child's where it did): P of the bar.  Returns the dict ``bounds`` reads, with Y and the ties of kind (2)."""
    M, N = G.shape
    rows, r_all, b_all = used_rows(mu, sigma, keep)
    Gk, r, b = G[rows].astype(np.int64), r_all[rows], b_all[rows]
    z = draw(rows, M, l, seed, offset, mutate)
    zf = z if mutate == "z_f64" else z.astype(np.float32)
    T = r.astype(np.float64)[:, None] * z if mutate == "z_f64" else r[:, None] * zf          # (f32 * f32 in numpy: one rounding, as __fmul_rn)
    assert mutate == "z_f64" or T.dtype == np.float32
    rmax = float(np.max(r, initial=np.float32(0)))
    if mutate == "rmax_all_rows":
        ok = np.abs(sigma) >= np.float32(1e-9)
        rmax = float(np.max(np.float32(1) / sigma[ok]))
        assert rmax > float(np.max(r))
    bound, S = 6.67 * rmax, digit_scale(nd)
    t = T.astype(np.float64) * (S / bound)
    v = np.rint(t).astype(np.int64)
    near = np.abs(np.abs(t - np.floor(t)) - 0.5) <= 4 * np.spacing(np.abs(t))
    for i, j in np.argwhere(near):                             # (a few entries: rational arithmetic on the constants as the source writes them)
        exact = Fraction(float(T[i, j])) * Fraction(49, 100) * (256 ** 3 if nd == 3 else 128 ** 4) / (Fraction(667, 100) * Fraction(rmax))
        near[i, j] = (2 * exact).denominator != 1 or (2 * exact).numerator % 2 == 0
    ties1 = np.sum(near, axis=0)
    tie2 = f32_boundary_ties(z)
    digits_ok = True
    if mutate == "base128_at_nd3":
        assert nd == 3
        dg, _ = split_digits(v, 4, wrap=True)                  # (k_omega's other branch; K2 reads three planes in base 256)
        Yint = sum(int_dot(Gk, d) * 256 ** i for i, d in enumerate(dg[:3]))
    else:
        lim = (128, 127) if nd == 3 else (64, 63)
        dg, base = split_digits(v, nd)
        digits_ok = all(int(d.min(initial=0)) >= -lim[0] and int(d.max(initial=0)) <= lim[1] for d in dg)
        assert np.array_equal(sum(d * base ** i for i, d in enumerate(dg)), v)
        Yint = int_dot(Gk, v)
    if mutate == "one_unit":
        Yint[N // 2, col] += 1
    ld = np.longdouble
    Tb = b.astype(np.float64)[:, None] * zf.astype(np.float64)             # (exact in f64 where zf is f32)
    in_c = rows < (M - 1) // 64 * 64 if mutate == "last_group_out_of_c" else np.ones(len(rows), bool)
    c = np.sum(Tb[in_c].astype(ld), axis=0)
    sa = np.full(l, bound / S)
    Y = (sa.astype(ld)[None, :] * Yint.astype(ld) + c[None, :]).astype(np.float64)
    gk = Gk.astype(np.float64)
    k0, z1 = np.zeros(l), np.zeros((1, l))
    return dict(Y=Y, c=c.astype(np.float64), sa=sa, sb=k0, Yia=Yint, Yib=z1, Ta=T, Tb=Tb, ties_a=ties1, ties_b=k0, ga=gk, miss=np.zeros((1, 1)),
                M=M if rows_run is None else rows_run, digits_ok=digits_ok, rows=rows, z=z,
                ties_z=tie2.sum(axis=0), ztie_bar=2 * U32 * (gk.T @ (np.abs(T.astype(np.float64)) * tie2)))


def sketch_bounds(m):
    """(bar against the model, bar against the truth), both [N][l]: ``bounds`` plus the ties of kind (2) and the third u32 sum |g Ta|"""
    bm, bt = bounds(m, True)
    return bm + m["ztie_bar"], bt + m["ztie_bar"] + U32 * (m["ga"].T @ np.abs(m["Ta"].astype(np.float64)))


def sketch_truth(G, mu, sigma, m):
    rows = m["rows"]
    A = (G[rows].astype(np.float64) - mu[rows].astype(np.float64)[:, None]) / sigma[rows].astype(np.float64)[:, None]
    return A.T @ m["z"]


def few_ties(m):
    return np.mean((m["ties_a"] == 0) & (m["ties_z"] == 0)) >= 0.95


def assert_one_unit_is_visible(m, what):
    """a tie-free column exists, and its bar against the model is below a quarter of one integer unit bound / S at every sample"""
    free = np.flatnonzero((m["ties_a"] == 0) & (m["ties_z"] == 0))
    assert len(free) > 0, what + ": no tie-free column"
    assert not np.any(m["Tb"]), what + ": zero_mu leaves no c"
    worst = float(np.max(sketch_bounds(m)[0][:, free] / m["sa"][None, free]))
    assert worst < 0.25, f"{what}: the bar is {worst:.3g} units of Yint wide"
    return free


def f32_sketch_model(G, mu, sigma, keep, l, seed, offset, packed):
    """(truth, bar) of the sketch on GPCA_PREC_F32_MFMA: the f32 pass of test_gpu_k2_pass.py with W = zf on the rows used"""
    M, N = G.shape
    rows, r, _ = used_rows(mu, sigma, keep)
    z = draw(rows, M, l, seed, offset)
    assert not np.any(np.all(z.astype(np.float32) == 0, axis=1))
    W = np.zeros((M, l), np.float32)
    W[rows] = z.astype(np.float32)
    truth, bar = f32_pass_model(G, mu, sigma, W, f32_plan(M, N, packed))      # (the launched plan: Npad is 1024-padded on 2-bit rows)
    tie2 = f32_boundary_ties(z)
    T = np.abs(r[rows].astype(np.float64)[:, None] * z)
    return truth, bar + 2 * U32 * (G[rows].astype(np.float64).T @ (T * tie2)), tie2.sum(axis=0)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
_STD = {}


def standardisation(family, M, keepname, keep):
    """(mu, sigma) of a family, seeded per (family, M, keep).  Where the largest r sits: every row -- row 0 under zero_mu, row M - 1 under
    small_mu; last block dropped -- the last kept row, and a larger 1 / sigma still on the dropped last row; one row -- a larger 1 / sigma
    on the dropped row 0."""
    key = (family, M, keepname)
    if key not in _STD:
        rng = np.random.default_rng([M, FAMILIES.index(family), len(keepname)])
        if family == "zero_mu":                                # (the generic rows 1 .. 1/8, the two singled out below 1/16 and 1/32)
            mu, sigma, top, over = np.zeros(M, np.float32), (2.0 ** -rng.integers(0, 4, M)).astype(np.float32), np.float32(1 / 16), np.float32(1 / 32)
        else:                                                  # (rmax no power of two: no rational structure in S / bound)
            mu, sigma = rng.uniform(0.002, 0.02, M).astype(np.float32), np.exp(rng.uniform(np.log(1 / 16), 0.0, M)).astype(np.float32)
            top, over = np.float32(1 / 19.3), np.float32(1 / 1930.0)      # (the dropped row's 1 / sigma 100 x the kept maximum: see TEETH)
        kept = np.flatnonzero(keep)
        if keepname == "last block dropped":
            sigma[kept[-1]], sigma[M - 1] = top, over
        elif keepname == "one row":
            sigma[kept[0]] = top
            if M > 1:
                sigma[0] = over
        elif keepname == "seventh":                            # (row 3 dropped; row M - 1 kept: alone in the last wave at 4097 rows)
            assert keep[M - 1] and not keep[3]
            sigma[M - 1], sigma[3] = top, over
        else:
            sigma[0 if family == "zero_mu" else M - 1] = top
        _STD[key] = (mu, sigma)
    return _STD[key]


def seventh_dropped(M):
    keep = np.ones(M, np.uint8)
    keep[3::7] = 0
    return keep


def child_keep(M):
    """every third row kept, irregularly: each row with probability 1 / 3"""
    return (np.random.default_rng(3).random(M) < 1 / 3).astype(np.uint8)


def child_standardisation(family, M):
    rng = np.random.default_rng([M, FAMILIES.index(family)])
    if family == "zero_mu":
        return np.zeros(M, np.float32), (2.0 ** -rng.integers(0, 6, M)).astype(np.float32)
    return rng.uniform(0.002, 0.02, M).astype(np.float32), np.exp(rng.uniform(np.log(1 / 32), 0.0, M)).astype(np.float32)


# ---- teeth (CPU) -------------------------------------------------------------------------------------------------------------------------------
MUTANTS = ["last_wave_zero", "seed_high_dropped", "last_column_zero", "pair_swapped", "rmax_all_rows", "one_unit", "z_f64", "last_group_out_of_c",
           "base128_at_nd3", "local_index", "index_high_dropped"]


def run_teeth(G, mu, sigma, keep, l, seed, offset, nd, family, mutants, what):
    m = sketch_model(G, mu, sigma, keep, l, seed, offset, nd)
    assert m["digits_ok"] and few_ties(m), what
    bar, bar_truth = sketch_bounds(m)
    assert np.all(np.abs(m["Y"] - sketch_truth(G, mu, sigma, m)) <= bar_truth), what + ": the model leaves the bar against the truth"
    col = int(assert_one_unit_is_visible(m, what)[0]) if family == "zero_mu" else 0
    for mut in mutants:
        if mut == "base128_at_nd3" and nd != 3:
            continue
        d = np.abs(sketch_model(G, mu, sigma, keep, l, seed, offset, nd, mutate=mut, col=col)["Y"] - m["Y"])
        f = fraction(d, bar)
        print(f"{what}: mutant {mut}: max |dY| / bar = {f:.3g}")
        if family == "small_mu" and mut in ("one_unit", "z_f64"):
            continue                                           # (recorded: the f32 term of c may hide a few units there)
        if family == "zero_mu" and mut == "last_group_out_of_c":
            assert np.all(d == 0)                              # (c is identically zero: nothing to leave out)
            continue
        assert np.any(d > bar), f"{what}: the bar lets the mutant '{mut}' through ({f:.3g} of it)"


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("nd", [3, 4])
def test_the_bar_rejects_every_mutant(nd, family):
    """4097 x 300, l = 33, every seventh row dropped with the largest 1 / sigma on a dropped row and the largest r on row 4096, alone in
    the last wave; the seed with its high word set"""
    M, N, l = 4097, 300, 33
    keepname, keep = "seventh", seventh_dropped(M)
    mu, sigma = standardisation(family, M, keepname, keep)
    run_teeth(genotypes(M, N), mu, sigma, keep, l, SEEDS[1], 0, nd, family, MUTANTS[:9], f"teeth nd={nd} {family}")


@pytest.mark.parametrize("family", FAMILIES)
def test_the_bar_rejects_the_straddle_mutant(family):
    M, N, l, off = 129, 300, 33, (1 << 32) - 40
    keep = np.ones(M, np.uint8)
    mu, sigma = standardisation(family, M, "every row", keep)
    for nd in (3, 4):
        muts = ["index_high_dropped", "last_wave_zero"]
        run_teeth(genotypes(M, N), mu, sigma, keep, l, SEEDS[0], off, nd, family, muts, f"straddle nd={nd} {family}")


@pytest.mark.parametrize("family", FAMILIES)
def test_the_bar_rejects_the_local_index_mutant(family):
    M, N, l = 70_000, 300, 33
    keep = child_keep(M)
    mu, sigma = child_standardisation(family, M)
    run_teeth(genotypes(M, N), mu, sigma, keep, l, SEEDS[0], 0, 4, family, ["local_index", "one_unit"], f"child {family}")


def test_the_f32_bar_rejects_gross_mutants():
    """GPCA_PREC_F32_MFMA: the chain bar sees a zeroed wave, a zeroed column and a swapped pair (and, by construction, no single unit)"""
    M, N, l = 4097, 300, 33
    keepname, keep = "seventh", seventh_dropped(M)
    for family in FAMILIES:
        mu, sigma = standardisation(family, M, keepname, keep)
        G = genotypes(M, N)
        rows, r, b = used_rows(mu, sigma, keep)
        for packed in (False, True):                           # (the plans of int8 and of 2-bit rows)
            truth, bar, tz = f32_sketch_model(G, mu, sigma, keep, l, 7, 0, packed)
            assert np.mean(tz == 0) >= 0.95
            for mut in ("last_wave_zero", "last_column_zero", "pair_swapped"):
                z = draw(rows, M, l, 7, 0, mut).astype(np.float32)
                cz = np.sum((b[rows][:, None] * z).astype(np.float64), axis=0)
                y = G[rows].astype(np.float64).T @ (r[rows][:, None] * z).astype(np.float64) + cz
                assert np.any(np.abs(y - truth) > bar), mut


# ---- the device --------------------------------------------------------------------------------------------------------------------------------
def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def device_sketch(e, N, l, seed):
    Y = np.full((N, l), np.nan)
    flag = C.c_int32(-1)
    e._chk(_lib.load().gpca_device_sketch(e._h, l, C.c_uint64(seed), _vp(Y), C.byref(flag)))
    return Y, flag.value


def open_engine(mode, **kw):
    prec, store, planes, _, _ = MODES[mode]
    return gpca.GpcaEngine(precision=prec, storage=store, digit_planes=planes, **kw)


def set_offset(e, offset, called):
    def hook(buf):
        called.append(len(buf))
    e.set_allreduce_hook(hook, 1, 0, offset)


def record(mode, family, f):
    RECORD[(mode, family)] = max(RECORD.get((mode, family), 0.0), f)
    print(f"    largest fraction of the bar against the model so far, {mode} {family}: {RECORD[(mode, family)]:.3g}")


def check_sketch(Y, G, mu, sigma, keep, l, seed, offset, mode, family, what, rows_run=None):
    nd = MODES[mode][3]
    assert Y.shape == (G.shape[1], l) and np.all(np.isfinite(Y)), what
    if nd:
        m = sketch_model(G, mu, sigma, keep, l, seed, offset, nd, rows_run=rows_run)
        assert m["digits_ok"] and few_ties(m), what + ": the seeded input ties too often: change the seed"
        if family == "zero_mu":
            assert_one_unit_is_visible(m, what)
        bar, bar_truth = sketch_bounds(m)
        d, dt = np.abs(Y - m["Y"]), np.abs(Y - sketch_truth(G, mu, sigma, m))
        f, ft = fraction(d, bar), fraction(dt, bar_truth)
        print(f"{what}: max |Y_device - Y_model| / bar = {f:.3g}, max |Y_device - Y_truth| / bar = {ft:.3g}")
        assert np.all(d <= bar), f"{what}: {f:.3g} of the bar against the model"
        assert np.all(dt <= bar_truth), f"{what}: {ft:.3g} of the bar against the truth"
    else:
        truth, bar, tz = f32_sketch_model(G, mu, sigma, keep, l, seed, offset, MODES[mode][4])
        assert np.mean(tz == 0) >= 0.95, what
        d = np.abs(Y - truth)
        f = fraction(d, bar)
        print(f"{what}: max |Y_device - Y_truth| / bar = {f:.3g}")
        assert np.all(d <= bar), f"{what}: {f:.3g} of the bar"
    record(mode, family, f)
    return f


def run_case(mode, G, mu, sigma, keep, l, seed, family, what, offset=0, **kw):
    """one resident handle, one sketch; a refusal where preflight demands one (l > N, l > kept rows without an offset, l > 64 on f32)"""
    M, N = G.shape
    kept = int(len(used_rows(mu, sigma, keep)[0]))
    with open_engine(mode, **kw) as e:
        e.upload_genotypes_i8(G)
        e.set_standardization(mu, sigma, keep)
        called = []
        if offset:
            set_offset(e, offset, called)
        refuse = N < 2 or l > N or (not offset and l > kept) or (l > 64 and not MODES[mode][3])
        if refuse:
            with pytest.raises(_lib.GpcaError) as ex:
                device_sketch(e, N, l, seed)
            assert ex.value.status == _lib.GPCA_ERR_BAD_ARG, what
            return None
        Y, on_child = device_sketch(e, N, l, seed)
        Y2, _ = device_sketch(e, N, l, seed)
        assert _lib.load().gpca_get_scores(e._h, _vp(np.zeros((N, l), np.float32))) == _lib.GPCA_ERR_STATE      # (the hook leaves have_rsvd false)
    assert on_child == 0 and not called and np.array_equal(Y, Y2), what
    check_sketch(Y, G, mu, sigma, keep, l, seed, offset, mode, family, what)
    return Y


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("M", [1, 63, 64, 65, 127, 128, 129, 4097])
def test_sketch_rows_and_keep_masks(mode, M):
    """the wave's live edge, the pad rows, every keep mask of edge_keeps; l = 33 (two column halves) where the kept rows allow it"""
    N = 300
    G = genotypes(M, N)
    for n, (keepname, keep) in enumerate(edge_keeps(M)):
        for f, family in enumerate(FAMILIES):
            mu, sigma = standardisation(family, M, keepname, keep)
            l = min(33, int(keep.sum()))
            run_case(mode, G, mu, sigma, keep, l, SEEDS[(n + f) % 2], family, f"sketch {mode} {family} M={M} '{keepname}' l={l}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("N", [5, 300])
@pytest.mark.parametrize("l", [1, 31, 32, 33, 64, 65, 100, 128])
def test_sketch_widths(mode, l, N):
    """the three instantiations of k_omega and partial quads; columns >= l must not contribute (the hook returns l columns of L; a column
    >= l that leaked into c or the planes would show in none of them, one that displaced a column < l in all)"""
    M = 194                                                    # (three waves and two rows; row 3 dropped, row 193 kept)
    keep = seventh_dropped(M)
    G = genotypes(M, N)
    for f, family in enumerate(FAMILIES):
        mu, sigma = standardisation(family, M, "seventh", keep)
        run_case(mode, G, mu, sigma, keep, l, SEEDS[(l + f) % 2], family, f"sketch {mode} {family} N={N} l={l}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("offset,M", [(5, 193), ((1 << 32) - 40, 129)])
def test_sketch_snp_offset(mode, offset, M):
    N, l = 300, 33
    keep = np.ones(M, np.uint8)
    G = genotypes(M, N)
    for f, family in enumerate(FAMILIES):
        mu, sigma = standardisation(family, M, "every row", keep)
        run_case(mode, G, mu, sigma, keep, l, SEEDS[f], family, f"sketch {mode} {family} M={M} snp_offset={offset}", offset=offset)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("mode", ["int8", "2bit"])
def test_sketch_compact_child(mode, family):
    M, N, l, seed = 70_000, 300, 33, SEEDS[0]
    G, keep = genotypes(M, N), child_keep(M)
    mu, sigma = child_standardisation(family, M)
    n_kept = int(keep.sum())
    out = {}
    for flags in (0, _lib.CFG_NO_COMPACT):
        with open_engine(mode, flags=flags) as e:
            e.upload_genotypes_i8(G)
            e.set_standardization(mu, sigma, keep)
            out[flags] = device_sketch(e, N, l, seed)
    assert out[0][1] == 1 and out[_lib.CFG_NO_COMPACT][1] == 0
    check_sketch(out[0][0], G, mu, sigma, keep, l, seed, 0, mode, family, f"compact child {mode} {family}", rows_run=n_kept)
    check_sketch(out[_lib.CFG_NO_COMPACT][0], G, mu, sigma, keep, l, seed, 0, mode, family, f"parent, no child {mode} {family}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", EXACT)
def test_sketch_streamed_panels(mode):
    """4097 rows in panels of 2048: the last panel holds one row.  Every seventh row dropped: row 4096 is kept and carries the largest r,
    so a last panel skipped or read at a wrong plane offset (row0 >> 5) leaves the model; last block dropped: that panel is all-dropped
    and must add nothing.  Fused on and off and the resident handle give the same bits (the sketch's scale is the same for every panel)"""
    M, N, l, seed = 4097, 300, 33, SEEDS[1]
    G = genotypes(M, N)
    for keepname, keep in (("seventh", seventh_dropped(M)), edge_keeps(M)[1]):
        assert bool(keep[M - 1]) == (keepname == "seventh")
        for family in FAMILIES:
            mu, sigma = standardisation(family, M, keepname, keep)
            assert keepname != "seventh" or sigma[M - 1] == np.min(sigma[keep == 1])
            Y = run_case(mode, G, mu, sigma, keep, l, seed, family, f"sketch resident {mode} {family} '{keepname}'")
            for fused in (True, False):
                with open_engine(mode) as e:
                    e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), M, N, panel_rows=2048, ring_slots=2, fused=fused)
                    assert e.stream_info()["n_panels"] == 3
                    e.set_standardization(mu, sigma, keep)
                    Ys, on_child = device_sketch(e, N, l, seed)
                assert on_child == 0 and np.array_equal(Ys, Y), f"streamed fused={fused} {mode} {family} '{keepname}'"


@pytest.mark.gpu
@pytest.mark.parametrize("mode,l", [("int8", 33), ("2bit", 100)])
def test_rsvd_runs_the_same_sketch(mode, l):
    """gpca_rsvd(l, 0, 0, seed): span(scores) = span(Y) -- the span identity, against the model's Y"""
    M, N, seed, family = 4097, 300, SEEDS[1], "zero_mu"
    G = genotypes(M, N)
    keepname, keep = edge_keeps(M)[1]
    mu, sigma = standardisation(family, M, keepname, keep)
    m = sketch_model(G, mu, sigma, keep, l, seed, 0, MODES[mode][3])
    Yt = sketch_truth(G, mu, sigma, m)
    cond = float(np.linalg.cond(Yt))
    assert cond ** 2 * U64 < 1, "CholeskyQR needs cond(Y)^2 u64 < 1"
    with open_engine(mode) as e:
        e.upload_genotypes_i8(G)
        e.set_standardization(mu, sigma, keep)
        e.rsvd(l, 0, 0, seed=seed)
        S = e.scores(f64=True)
    assert S.shape == (N, l) and np.all(np.isfinite(S))
    count = 2 * l * np.sqrt(l) * cond + (l + 2) * np.sqrt(l) + 2 * N
    bar = np.linalg.norm(sketch_bounds(m)[0], axis=0) + count * U64 * np.linalg.norm(m["Y"], axis=0)
    Pn, _ = np.linalg.qr(S)
    res = np.linalg.norm(m["Y"] - Pn @ (Pn.T @ m["Y"]), axis=0)
    f = fraction(res, bar)
    print(f"span identity {mode} l={l}: cond(Y) = {cond:.3g}, largest residual / bar = {f:.3g}")
    assert np.all(res <= bar), f"{f:.3g} of the bar"
