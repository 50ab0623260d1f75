"""K2 inside the fused streamed power sweep (stage_power_fused: launch_quantize_f32_premax per panel, k2_panel, launch_accum_y_scaled,
launch_finish_y_sum), held per element to a bar derived from its arithmetic -- through the test hook gpca_device_power (include/gpca.h),
which uploads a sketch, runs stage_orth(2) and then ONE power iteration exactly as gpca_rsvd chooses it for the handle, and returns
Q (the f64 basis), Tq (T' = r o (A Q), f32, as K2 reads it), c and the new sketch.  Style of test_gpu_k2_pass.py.

TRUSTED INPUT.  Tq is the input of the stage under test and is taken as given, as test_gpu_k2_pass.py takes the loadings (K1 has its own
module, test_gpu_k1_pass.py).  Q is held only to |Q^T Q - I| under the dense chain's bar (test_gpu_dense_chain.orth_fractions).  c is NOT
trusted: c_j = -sum_i mu_i Tq_ij within u32 (64 + 3) sum_i |mu_i Tq_ij| -- the f32 term of ``bounds`` (64-row f32 partials) plus the
roundings of b, r and the quotient -- and exactly 0 under zero_mu; once held, the device's c enters the model of Y.

THE MODEL (``panel_model``; from stage_power_fused and fold_quantize_i8.hip).  For every panel p, rows [row0_p, row0_p + rows_p):
    colmax_pj = max_i |Tq_ij| over the panel,   q = rint(Tq S / colmax_pj),   Yint_p = G_p^T q  exactly,
    Y = sum_p (colmax_pj / S) Yint_p + c                    S = 0.49 * 128^4 (4 planes) or 0.49 * 256^3 (3 planes)
(k_accum_y_scaled: one fma per panel in panel order, the first panel onto 0; k_finish_y_sum: c added last).  A panel whose kept rows are
all dropped has colmax = 0: its scale is 0 and nothing is added.
THE BAR:  u64 (panels + P + 2) (sum_p |scale_p Yint_p| + |c_j| + sum_i |mu_i Tq_ij|)  +  the counted ties (an entry of Tq S / colmax
within 4 ulp of a half-integer: one unit scale_pj each), P = ceil(Mpad / 64); at least 95 % of the (panel, column) pairs are tie-free,
asserted on the CPU before any comparison.  Under zero_mu (test_gpu_sketch_pass.py's family) c = 0 and the bar is u64 (panels + P + 2) sum_p |..|;
every zero_mu case asserts that in a tie-free column it is below a QUARTER of the unit scale_pj of every panel: one wrong integer in any
panel's tile shows.
With gpca_stream_set_fused(h, 0) the same hook runs stage_AQ over all panels and then stage_AtT_local: the model is the same with ONE
panel of all rows (the global column maxima: exact_pass_model's side a), and Q, Tq, c and Yout equal a resident handle's bit for bit.

SHAPES.  4097 rows; panel_rows 128 (the smallest gpca_stream_open accepts: 33 panels) and 2048 (3 panels); either way the last panel
holds one row -- row 4096 carries the largest r, so that its unit is not the smallest.  N in {200, 300}: the narrow and the wide kernels
on int8 rows; 2-bit rows with 3 and 4 planes.  l in {10, 33}: l = 33 runs two column halves, the second half's scales sit at + 32.
Keep masks: every seventh row dropped; and, at panel_rows 2048, every row of the middle panel dropped as well.  One sketch makes column 0
of T' zero inside the first panel only (its Q column lives on four samples whose dosages are 0 in that panel).  Every handle runs twice:
the same bits (the accumulators are reset by the first panel, pv.index == 0).

TEETH (CPU, unmarked; Tq from an f64 K1 on the device cases' own inputs).  Each mutant of ``MUTANTS`` leaves the bar: panel p added
with panel p - 1's scale; the first panel's sums not reset on a second call; the all-dropped panel contributing stale planes with the
previous scale; the second column half using the first half's scales; the last one-row panel left out; and the global colmax used on
the fused handle (required under zero_mu: the test tells the two grids apart; recorded under small_mu).

Not reached: a fault of K1 that Tq itself carries (test_gpu_k1_pass.py's business); an error common to the model and the kernels.

Measured on one MI355X, the largest fraction of the bar over every case, sample and column (records, not thresholds; each test prints
its own with -s):
    zero_mu:   int8 0.069, 2-bit (3 planes) 0.059, 2-bit (4 planes) 0.069          small_mu:  0.052 / 0.054 / 0.052
    c against -mu^T Tq: 0.0038 of its bar;  Q, Tq, c and Yout of the unfused streamed handle equal the resident handle's in every case
The module's wall time there: 5 s for its 50 device cases; the 12 CPU cases take 2 s.
One value-only defect compiled into stage_power_fused on a scratch copy (launch_accum_y_scaled given d_tscale without + 32 hf: the
second column half scaled by the first half's scales), run once: all 24 cases with l = 33 went red, all 24 with l = 10 and the
refusal of a sharded handle stayed green; of test_streamed_fused_power_iteration the two k = 40 cases went red too and the three
k = 10 cases stayed green, as did test_streamed_equals_resident_bitwise and test_transform_streamed_panels (neither runs the fused
sweep past 32 columns).
"""
import ctypes as C

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from test_gpu_dense_chain import orth_fractions, precondition
from test_gpu_exact_pass import U32, U64, int_dot, quantize
from test_gpu_k2_pass import MODES, EXACT, fraction, genotypes
from test_gpu_sketch_pass import FAMILIES, seventh_dropped, standardisation

M_ROWS = 4097
RECORD = {}


def panels_of(M, panel_rows):
    return [(r0, min(r0 + panel_rows, M)) for r0 in range(0, M, panel_rows)]


def keep_mask(name, M):
    keep = seventh_dropped(M)
    if name == "middle":
        keep[2048:4096] = 0
    return keep


def sketch_input(N, l, zero_col=False):
    rng = np.random.default_rng([N, l])
    Y = rng.standard_normal((N, l))
    if zero_col:
        Y[:, 0] = 0
        Y[:4, 0] = [1.0, -2.0, 3.0, 1.0]
    return Y


def genotypes_for(M, N, zero_col=False):
    G = genotypes(M, N)
    if zero_col:
        G = G.copy()
        G[:2048, :4] = 0
    return G


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
MUTANTS = ["neighbour_scale", "first_not_reset", "dropped_panel_stale", "second_half_first_scales", "last_panel_out", "global_colmax"]


def panel_model(G, mu, Tq, c, nd, panels, mutate=None):
    """Y [N][l] of the per-panel fixed point, its bar, and what the quarter-unit property reads (module docstring)"""
    M, N = G.shape
    l = Tq.shape[1]
    if mutate == "global_colmax":
        panels = [(0, M)]
    ld = np.longdouble
    acc, absacc, tiebar = np.zeros((N, l), ld), np.zeros((N, l)), np.zeros(l)
    scales, ties, prev = [], [], None
    for p, (r0, r1) in enumerate(panels):
        if mutate == "last_panel_out" and p == len(panels) - 1:
            continue
        q, scale, t = quantize(Tq[r0:r1], nd)
        Yi = int_dot(G[r0:r1].astype(np.int64), q)
        use = scale
        if mutate == "neighbour_scale" and p > 0:
            use = prev[1]
        if mutate == "dropped_panel_stale" and p > 0 and not np.any(Tq[r0:r1]):
            use, Yi = prev[1], int_dot(G[r0:r1].astype(np.int64), prev[0][:r1 - r0])      # (the planes the panel before left, its scale)
        if mutate == "second_half_first_scales" and l > 32:
            use = use.copy(); use[32:] = use[:l - 32]
        acc += use.astype(ld)[None, :] * Yi.astype(ld)
        absacc += np.abs(use[None, :] * Yi)
        tiebar += t * scale
        scales.append(scale); ties.append(t)
        prev = (q, scale)
    if mutate == "first_not_reset":
        acc = acc + acc
    sum_tb = np.sum(np.abs(mu.astype(np.float64)[:, None] * Tq.astype(np.float64)), axis=0)
    P = ((M + 127) // 128 * 128 + 63) // 64
    Y = (acc + c.astype(ld)[None, :]).astype(np.float64)
    bar = U64 * (len(panels) + P + 2) * (absacc + (np.abs(c) + sum_tb)[None, :]) + tiebar[None, :]
    return dict(Y=Y, bar=bar, scales=np.array(scales), ties=np.array(ties))


def few_ties(m):
    return np.mean(m["ties"] == 0) >= 0.95


def assert_one_unit_is_visible(m, what):
    """a tie-free column exists, and the bar there is below a quarter of the unit of every panel that has one"""
    free = np.flatnonzero(np.all(m["ties"] == 0, axis=0) & np.any(m["scales"] > 0, axis=0))
    assert len(free) > 0, what + ": no tie-free column"
    unit = np.min(np.where(m["scales"] > 0, m["scales"], np.inf), axis=0)
    worst = float(np.max(m["bar"][:, free] / unit[None, free]))
    assert worst < 0.25, f"{what}: the bar is {worst:.3g} units of the finest panel grid wide"


def c_check(c, mu, Tq, what):
    ref = -np.sum(mu.astype(np.longdouble)[:, None] * Tq.astype(np.longdouble), axis=0).astype(np.float64)
    bar = U32 * (64 + 3) * np.sum(np.abs(mu.astype(np.float64)[:, None] * Tq.astype(np.float64)), axis=0)
    f = fraction(np.abs(c - ref), bar)
    print(f"{what}: max |c - (-mu^T Tq)| / bar = {f:.3g}")
    assert np.all(np.abs(c - ref) <= bar), f"{what}: c at {f:.3g} of its bar"
    return f


def cpu_k1(G, mu, sigma, keep, Yin):
    """(Tq f32 [M][l], c [l]) of an f64 K1 on the CPU: the input of the teeth"""
    Q, _ = np.linalg.qr(Yin)
    r = np.where(keep.astype(bool), 1.0 / sigma.astype(np.float64), 0.0)
    T = (r[:, None] * ((G.astype(np.float64) - mu.astype(np.float64)[:, None]) @ Q)).astype(np.float32)
    return T, -np.sum(mu.astype(np.float64)[:, None] * T.astype(np.float64), axis=0)


# ---- teeth (CPU) -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("nd", [3, 4])
@pytest.mark.parametrize("panel_rows,keepname", [(128, "seventh"), (2048, "seventh"), (2048, "middle")])
def test_the_bar_rejects_every_mutant(panel_rows, keepname, nd, family):
    M, N, l = M_ROWS, 300, 33
    G, keep = genotypes(M, N), keep_mask(keepname, M)
    mu, sigma = standardisation(family, M, "seventh", seventh_dropped(M))
    Tq, c = cpu_k1(G, mu, sigma, keep, sketch_input(N, l))
    panels = panels_of(M, panel_rows)
    m = panel_model(G, mu, Tq, c, nd, panels)
    assert few_ties(m)
    if family == "zero_mu":
        assert not np.any(c)
        assert_one_unit_is_visible(m, "teeth")
    if keepname == "middle":
        assert not np.any(m["scales"][1]) and np.all(m["scales"][[0, 2]] > 0)
    for mut in MUTANTS:
        if mut == "dropped_panel_stale" and keepname != "middle":
            continue
        d = np.abs(panel_model(G, mu, Tq, c, nd, panels, mutate=mut)["Y"] - m["Y"])
        f = fraction(d, m["bar"])
        print(f"panel_rows={panel_rows} {keepname} nd={nd} {family}: mutant {mut}: max |dY| / bar = {f:.3g}")
        if mut == "global_colmax" and family == "small_mu":
            continue                                           # (recorded: another grid moves Y by the quantisation noise only)
        assert np.any(d > m["bar"]), f"the bar lets the mutant '{mut}' through ({f:.3g} of it)"


# ---- the device --------------------------------------------------------------------------------------------------------------------------------
def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def device_power(e, M, N, Yin):
    l = Yin.shape[1]
    Yin = np.ascontiguousarray(Yin, np.float64)
    Q, Tq, c, Yout = np.full((N, l), np.nan), np.full((M, l), np.nan, np.float32), np.full(l, np.nan), np.full((N, l), np.nan)
    e._chk(_lib.load().gpca_device_power(e._h, _vp(Yin), l, _vp(Q), _vp(Tq), _vp(c), _vp(Yout)))
    assert _lib.load().gpca_get_scores(e._h, _vp(np.zeros((N, l), np.float32))) == _lib.GPCA_ERR_STATE      # (the hook leaves have_rsvd false)
    return Q, Tq, c, Yout


def open_engine(mode, **kw):
    prec, store, planes, _, _ = MODES[mode]
    return gpca.GpcaEngine(precision=prec, storage=store, digit_planes=planes, **kw)


def run_handle(mode, G, mu, sigma, keep, Yin, panel_rows, fused):
    """two calls on one handle (panel_rows 0: resident); the bits must repeat"""
    M, N = G.shape
    with open_engine(mode) as e:
        if panel_rows:
            e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), M, N, panel_rows=panel_rows, ring_slots=2, fused=fused)
            assert e.stream_info()["n_panels"] == len(panels_of(M, panel_rows))
        else:
            e.upload_genotypes_i8(G)
        e.set_standardization(mu, sigma, keep)
        a = device_power(e, M, N, Yin)
        b = device_power(e, M, N, Yin)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), "a second call on the same handle gave other bits"
    return a


def record(mode, family, f):
    RECORD[(mode, family)] = max(RECORD.get((mode, family), 0.0), f)
    print(f"    largest fraction of the bar so far, {mode} {family}: {RECORD[(mode, family)]:.3g}")


def check_power(out, G, mu, keep, Yin, nd, panels, family, what):
    Q, Tq, c, Yout = out
    assert all(np.all(np.isfinite(x)) for x in out), what
    precondition(Yin)
    fq = orth_fractions(Yin, Q, 2)["orthonormality"]
    assert fq <= 1, f"{what}: |Q^T Q - I| at {fq:.3g} of the dense chain's bar"
    assert not np.any(Tq[keep == 0]), what + ": rows QC dropped must be zero in T'"
    if family == "zero_mu":
        assert not np.any(c), what + ": c must be exactly 0 under zero_mu"
    else:
        c_check(c, mu, Tq, what)
    m = panel_model(G, mu, Tq, c, nd, panels)
    assert few_ties(m), what + ": the seeded input ties too often: change the seed"
    if family == "zero_mu":
        assert_one_unit_is_visible(m, what)
    d = np.abs(Yout - m["Y"])
    f = fraction(d, m["bar"])
    print(f"{what}: max |Y_device - Y_model| / bar = {f:.3g}")
    assert np.all(d <= m["bar"]), f"{what}: {f:.3g} of the bar"
    return m, f


def run_case(mode, N, l, panel_rows, keepname, family, zero_col=False):
    M, nd = M_ROWS, MODES[mode][3]
    G, keep = genotypes_for(M, N, zero_col), keep_mask(keepname, M)
    mu, sigma = standardisation(family, M, "seventh", seventh_dropped(M))
    Yin = sketch_input(N, l, zero_col)
    what = f"power {mode} {family} N={N} l={l} panel_rows={panel_rows} keep={keepname}" + (" zero column" if zero_col else "")
    fused = run_handle(mode, G, mu, sigma, keep, Yin, panel_rows, True)
    m, f = check_power(fused, G, mu, keep, Yin, nd, panels_of(M, panel_rows), family, what + " fused")
    record(mode, family, f)
    if keepname == "middle":
        assert not np.any(m["scales"][1]), what + ": the all-dropped panel must have scale 0"
    if zero_col:
        assert not np.any(fused[1][:2048, 0]) and np.any(fused[1][2048:, 0]), what + ": column 0 of T' must vanish in the first panel only"
        assert m["scales"][0][0] == 0 and np.all(m["scales"][0][1:] > 0)
    plain = run_handle(mode, G, mu, sigma, keep, Yin, panel_rows, False)
    check_power(plain, G, mu, keep, Yin, nd, [(0, M)], family, what + " unfused")
    resident = run_handle(mode, G, mu, sigma, keep, Yin, 0, False)
    for name, x, y in zip(("Q", "Tq", "c", "Yout"), plain, resident):
        assert np.array_equal(x, y), f"{what}: {name} of the unfused streamed handle differs from the resident handle's"
    assert np.array_equal(fused[0], resident[0]), what + ": Q does not depend on the sweep"
    if family == "zero_mu":                                    # (the test tells the two grids apart: the fused result is NOT the global-colmax one)
        g = panel_model(G, mu, fused[1], fused[2], nd, [(0, M)])
        assert np.any(np.abs(fused[3] - g["Y"]) > m["bar"]), what + ": the fused sweep sits inside the global-colmax model"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", EXACT)
@pytest.mark.parametrize("N", [200, 300])
@pytest.mark.parametrize("l", [10, 33])
@pytest.mark.parametrize("panel_rows,keepname", [(128, "seventh"), (2048, "seventh"), (2048, "middle")])
def test_fused_sweep_panels(mode, N, l, panel_rows, keepname):
    for family in FAMILIES:
        run_case(mode, N, l, panel_rows, keepname, family)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", EXACT)
@pytest.mark.parametrize("N", [200, 300])
@pytest.mark.parametrize("l", [10, 33])
def test_fused_sweep_column_zero_in_one_panel(mode, N, l):
    run_case(mode, N, l, 2048, "seventh", "zero_mu", zero_col=True)


@pytest.mark.gpu
def test_power_hook_refuses_the_f32_precision():
    """on GPCA_PREC_F32_MFMA K1 keeps T' blocked: the hook has no row-major Tq to return and says so"""
    M, N = 129, 300
    mu, sigma = standardisation("zero_mu", M, "every row", np.ones(M, np.uint8))
    for mode in ("f32", "f32_2bit"):
        with open_engine(mode) as e:
            e.upload_genotypes_i8(genotypes(M, N))
            e.set_standardization(mu, sigma, None)
            with pytest.raises(_lib.GpcaError) as ex:
                device_power(e, M, N, sketch_input(N, 10))
        assert ex.value.status == _lib.GPCA_ERR_STATE


@pytest.mark.gpu
def test_power_hook_refuses_a_sharded_handle():
    M, N = 129, 300
    mu, sigma = standardisation("zero_mu", M, "every row", np.ones(M, np.uint8))
    with open_engine("int8") as e:
        e.upload_genotypes_i8(genotypes(M, N))
        e.set_standardization(mu, sigma, None)
        e.set_allreduce_hook(lambda buf: None, 1, 0, 5)
        with pytest.raises(_lib.GpcaError) as ex:
            device_power(e, M, N, sketch_input(N, 10))
    assert ex.value.status == _lib.GPCA_ERR_STATE
