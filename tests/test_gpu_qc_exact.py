"""gpca_snp_stats (k_snp_stats in kernels.hip, k_snp_stats_2bit in store2bit.hip) and the producers that lay the genotype bytes down, held to
exact models at every edge of the sample axis, of the row axis and of the QC decisions.  Every routine above reads what this step writes.

THE MODEL (``Case``).  From the uploaded bytes alone, in Python integers and f64: nv = #(g != -127), n0 / n1 / n2 = #(g == 0 / 1 / 2),
s1 = sum g, s2 = sum g^2 over the valid calls as signed bytes (prepare.rs:1267-1279).  counts = (nv, n0, n1, n2) compare exactly.
mu = f32(f64(s1 / nv)) with s1 / nv the exact rational rounded once (Python's int / int is correctly rounded, as the kernel's one f64
division of two exact integers is); sigma = oracle.snp_sigma_exact: the exact rational (nv s2 - s1^2) / (nv (nv - 1)) rounded once to
f64, its square root, then f32.  The kernel forms nv s2 - s1^2 exactly (< 2^53), so sigma is asserted BIT-EQUAL, not within the ulp that
test_snp_stats_parity grants the two-pass oracle.  ``qc_reason`` restates reasons 1..6 of prepare.rs:1281-1364 in f64 in the kernel's
order (call rate, nv == 0, MAF, monomorphic, HWE, variance from (num / nv) / (nv - 1)); test_chain_restatement_equals_the_oracle holds it
to oracle.snp_stats on every matrix of this module.  keep, reason, num_pca_snps and pca_snp_rows compare exactly; mu and sigma are 0 on a
row that is not kept.  int8 and 2-bit residency must return the same bits.

A. THE SWEEP (``make_matrix``, seeded by (M, N)).  Rows: allele frequency log-uniform between a singleton 1 / 2N and 0.5, binomial
dosages, 3 % missing calls.  With M >= 12 rows 2..10 are planted: all 0, all 2, all missing, one valid call, two valid calls, alternating
0 / 2, all 1 (pfr = 0.5), missing exactly in the last sample, missing exactly in the first; below 12 rows the last M // 2 rows take
plants in turn.  Both kernels start their wave loads at the KiB boundary below the row start and the lanes in front of the row sit out;
rows cycle through the phases 0, 256, 512, 768 B.  A wrong lane count reads the tail of the rows in front, which is zero padding --
invisible -- unless the pitch has no pad: N = 256, 768, 1280 on int8, N = 1024, 3072, 5120 on 2-bit.  At those six sizes the last 16
(int8 sizes) or 64 (2-bit sizes) samples of every row but the planted nine are 2 (3 in 4) or missing (1 in 4): a stray read always adds
to nmiss, s1 and s2.  (The planted rows keep their pattern, or all 0 would not be all 0; the 122 other rows are dense.)  N_BOTH and
N_2BIT hold every trip boundary skip + vectors = 64 of either kernel and its neighbours; M = 131 gives every phase 32 times, a last workgroup
with three of four rows and a partial 32-row group; M in 1, 2, 3, 4, 5, 31, 32, 33 runs at N = 65, 768, 1025.  Each matrix is checked
under QcConfig.none(), QcConfig() and QcConfig(0.9, 0.05, 1e-3).  A row whose reference HWE p stands within the margin of section C of a
threshold would be left out of the keep / reason comparison; test_no_sweep_row_stands_near_an_hwe_threshold asserts there is none.

B. PRODUCERS.  The sweep's matrix at N = 5, 63, 257, 768, 1025 (3072 too on 2-bit), M = 131, through upload_genotypes_i8 (contiguous,
and as a column slice of a wider array filled with -127 and 2), upload_bed2bit (pad fields of the last byte set to 00 -> 2 and
01 -> missing), load_from_source (host_i8, host_bed, mapped_i8, mapped_bed) and a streamed handle of 128-row panels (the smallest
gpca_stream_open takes: two panels, the last of 3 rows, statistics written at row 128 on).  Same download, same statistics as in A.
Then once per residency, in one process: a handle filled with missing calls at 131 x 1280 is closed, and every producer runs on a fresh
handle at N = 1025 and N = 5 -- a pad column that kept the stale bytes would count as missing calls.

C. THE DEVICE HWE p.  hwe_p_dev and hwe_p_dev2 are hand copies of the host function and were seen only through keep on random rows.
Here K rows at N = 64 are built from genotype counts (n0, n1, n2) with 61..64 valid calls, laid out in shuffled sample order, sorted by
oracle.hwe_p; the thresholds are the geometric means of neighbouring p.  At each, exactly the rows below carry reason 5 and all others
are kept: the device p is pinned by rank between ~140 thresholds from 1e-13 to 1.  THE MARGIN of one p, with u = 2^-53:
    margin(p, chi) = (E + 2) u  +  p (chi / 2 + 8) 8 u
* absolute: the device erf is within E = 5 ulp of erf (HIP's documented bound), the reference's within 1, each ulp of a value below 1 is
  at most u; 1 - cdf is exact for cdf >= 1 / 2 and rounds by at most u / 2 below.
* relative: chi is a sum of three terms d^2 / e, each carrying at most 8 roundings (f, f f, f f tot, d, d d, the division, the sum, and
  one spare for a contracted multiply-subtract), so |delta chi| <= 8 u chi to first order; p = erfc(sqrt(chi / 2)) has
  |d ln p / d chi| <= 1 / 2 + 4 / chi on chi > 0 (the tail's log-slope), which gives p (chi / 2 + 4) 8 u; the bar doubles the constant.
* one term the formula leaves out: d = n - e cancels, so the 4 u e error of e enters chi as 8 u |d| <= 8 u N per term whatever chi is,
  |delta p| <= pdf(chi) 24 u N with pdf = exp(-chi / 2) / sqrt(2 pi chi).  ``first_order`` adds it.
The grid keeps every threshold at least 1000 margins AND twice first_order away from both neighbouring p (test_hwe_grid_is_separated;
a condition on the inputs, not a tolerance on the device); no row is skipped.  Rows with chi = 0 -- (16, 32, 16), (9, 30, 25),
(4, 24, 36), (1, 14, 49) and mirrors -- have p = 1 exactly in any arithmetic (every intermediate is dyadic) and are kept at every t < 1;
max_hwe_p = 1 drops nothing.  p = 0 EXACTLY CANNOT OCCUR AT 64 SAMPLES: chi = nv F^2 <= 64 (the infinite branches need e <= 1e-9 with
f >= 1e-9, that is 1e9 samples), and erf(sqrt(32)) = 1 - 1.2e-15 is below 1 (asserted on the CPU).  The p = 0 rows therefore live in a
companion matrix at N = 256 (chi from 114 to 256, erf saturated by 1e-23), beside rows with p = 1 and p around 0.1: at t = 0 exactly the
p = 0 rows drop, in the N = 64 matrix none does.
TEETH: ``hwe_chi_p`` is the function in Python f64 and reproduces oracle.hwe_p bit for bit on all 8 194 triples.  Four mutants -- eh without
the 2, c1 / c2 swapped with the hets left out, chi * 0.5 dropped, cdf for 1 - cdf -- each change the kept set at some threshold of the grid.
Two mutants CANNOT be told apart by any matrix below 1e9 samples and the test says so instead of pretending: a removed `else if ..
INFINITY` branch (unreachable, see above; told apart by calling the function at (1, 0, 1e9 - 1) against the host oracle) and a removed
p > 0 clamp (1 - erf(x) is never negative; equivalent on every triple).

D. EVERY BYTE VALUE.  1024 rows x 67 samples: row 4 v + j holds byte v at sample 16 q + 4 w + j -- every byte lane of a 32-bit word, with
sample 0 (odd v, j = 0) and the last sample 66 (odd v, j = 2) among the positions -- the rest random calls and a few missing.  int8:
counts, mu, sigma, keep, reason equal the signed byte-wise model (a row of {0, 1, 2, -127} is its own recount), rsvd is refused with -5
or -9.  Explicit 2-bit storage reports every invalid byte as a missing call and refuses rsvd; STORE_AUTO at N = 1024 with one invalid
byte ends on int8 with the int8 answer.  TEETH: ``fast_path_word`` restates the three mask expressions and vm on uint32 words; it
classifies all 256 values in all four lanes as the recount does, and three mutants (mask 0x7C7C7C78, m7 >> 7 dropped from vm,
~v & v >> 1) each get some value wrong.

E. DECISIONS AT EQUALITY, expected from ``qc_reason`` and pinned on the CPU: 49 / 50 = 0.98 and 9 / 10 = 0.9 kept, one more missing call
reason 1; maf = 0.05 from below 0.5 (s1 = 2 of 20 calls) kept, s1 = 1 reason 3; from above 0.5 the f64 value of 1 - 1.9 / 2 is
0.05000000000000004, not 0.05, so the row is held at min_maf = that value (kept) and one allele fewer gives reason 3; all-alt gives
reason 3 while min_maf > 0 and 4 at 0; one valid call reason 6; two equal calls 0, 0 or 2, 2 reason 4 (1, 1: reason 6).

F. standardize_block on the sweep's matrix at N = 5, 257, 1025: samples 0..4, N - 1 and every id next to a multiple of 4; rows = first
and last kept, one per KiB phase and the two planted rows with a missing call in sample 0 and N - 1; one request over all of them on the
samples none of them misses, and one per row on every sample that row has a call for, bit-equal to oracle.standardize_block; a request
that touches several missing calls gives -5 naming the first one in request order.

RECORDS (not thresholds).  On one MI355X the 91 device cases of this module pass and take 2.5 s of wall time together (the slowest, the
producers on recycled memory, 0.14 s); the 18 CPU tests take 4 s.  No row of any matrix stands near an HWE threshold, so nothing is
left out of any comparison, and the device agrees with the model in every bit: no defect was found in the kernels or the producers.
SEEDED DEFECTS, each compiled once into a scratch copy of both kernels and run once under section A (never committed):
* the lane in front of the row does not sit out (`if (v0 < skip - 1) continue;`): red at exactly the sizes whose pitch leaves less than
  one 16-byte vector of padding -- N = 255, 256, 767, 768, 1279, 1280 on int8, N = 1023, 1024, 3071, 3072, 5120 on 2-bit, and N = 768 at
  every M >= 2 -- and green at the other 42 cases, N = 769 among them.  No size the suite used before is in that list.
* `skip` forced to 0 (`const int64_t skip = 0;`, the window moves to the KiB boundary and loses the row's own tail): red at every size
  and every M >= 2, N = 769 included; green only at M = 1, where the one row starts on a boundary.  A defect that coarse was already
  visible to test_snp_stats_parity.
"""
import functools
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib

MISSING = -127
U = 2.0 ** -53
ERF_ULPS = 5                                   # HIP's documented bound for erf (tests/test_gpu_assoc_spa.py quotes the same)
STORES = {"int8": _lib.STORE_INT8, "2bit": _lib.STORE_2BIT}
QCS = (gpca.QcConfig.none(), gpca.QcConfig(), gpca.QcConfig(0.9, 0.05, 1e-3))

N_BOTH = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1279, 1280, 1281, 2047,
          2048, 2049]
N_2BIT = [3071, 3072, 3073, 4095, 4096, 4097, 5120]
PITCH_I8 = (256, 768, 1280)                    # ld8 == N
PITCH_2B = (1024, 3072, 5120)                  # ld2 == N / 4
M_SWEEP = 131
M_SMALL = [1, 2, 3, 4, 5, 31, 32, 33]
N_FOR_ROWS = [65, 768, 1025]
N_PRODUCERS = [5, 63, 257, 768, 1025]
N_BLOCK = [5, 257, 1025]
PANEL_ROWS = 128                               # kGQRowsPerWave: gpca_stream_open rounds panel_rows up to it


def _oracle():
    from oracle import oracle as O
    O.build()
    return O


# ---------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------
def hwe_chi_p(n_hom1, n_het, n_hom2, mut=None):
    """(chi, p) of prepare.rs:1641-1745 in Python f64, branch for branch (chi = None where the function returns before it has one).
    mut: one of HWE_MUTANTS (teeth only)"""
    tot = n_hom1 + n_het + n_hom2
    if tot == 0:
        return None, 1.0
    c1 = 2.0 * float(n_hom1) + float(n_het)
    c2 = 2.0 * float(n_hom2) + float(n_het)
    if mut == "swap_no_het":
        c1, c2 = 2.0 * float(n_hom2), 2.0 * float(n_hom1)
    ta = c1 + c2
    if ta <= 1e-9:
        return None, 1.0
    f1, f2 = c1 / ta, c2 / ta
    if f1 < 1e-9 or f2 < 1e-9:
        return None, 1.0
    if abs(f1 + f2 - 1.0) > 1e-6:
        return None, 1.0
    e1, eh, e2 = f1 * f1 * float(tot), 2.0 * f1 * f2 * float(tot), f2 * f2 * float(tot)
    if mut == "eh_without_2":
        eh = f1 * f2 * float(tot)
    chi = 0.0
    for k, (n, e) in enumerate(((n_hom1, e1), (n_het, eh), (n_hom2, e2))):
        if not math.isfinite(chi):
            break
        if e > 1e-9:
            d = float(n) - e
            chi += d * d / e
        elif float(n) > 1e-9 and not (mut == "no_inf_branch" and k == 0):
            chi = math.inf
    if math.isnan(chi):
        return chi, 1.0
    if chi == math.inf:
        return chi, 0.0
    cdf = math.erf(math.sqrt(chi if mut == "no_half" else chi * 0.5))
    if math.isnan(cdf):
        return chi, 1.0
    p = cdf if mut == "cdf_for_p" else 1.0 - cdf
    if mut == "no_clamp":
        return chi, p
    return chi, (p if p > 0.0 else 0.0)


HWE_MUTANTS = ("eh_without_2", "swap_no_het", "no_half", "cdf_for_p", "no_inf_branch", "no_clamp")
HWE_MUTANTS_THE_GRID_REJECTS = HWE_MUTANTS[:4]


def margin(p, chi):
    """the issue's margin of one device p (module docstring, section C)"""
    return (ERF_ULPS + 2) * U + p * ((chi or 0.0) / 2.0 + 8.0) * 8.0 * U


def first_order(p, chi, N):
    """margin's absolute term plus the cancellation term of d = n - e; chi = 0 (or none) is exact: every intermediate is dyadic"""
    if not chi:
        return (ERF_ULPS + 2) * U
    return (ERF_ULPS + 2) * U + math.exp(-chi / 2.0) / math.sqrt(2.0 * math.pi * chi) * (24.0 * N + 8.0 * chi) * U


def clear_of(t, p, chi, N):
    """is the threshold t at least 1000 margins and twice first_order away from the reference p?"""
    return abs(t - p) >= 1000.0 * margin(p, chi) and abs(t - p) >= 2.0 * first_order(p, chi, N)


def qc_reason(nv, n0, n1, n2, s1, s2, N, qc, hwe):
    """reasons 1..6 of prepare.rs:1281-1364 (0 = kept) in f64, in the order of k_snp_stats; hwe(n0, n1, n2) -> p"""
    if nv / N < qc.min_snp_call_rate:
        return 1
    if nv == 0:
        return 2
    mean = s1 / nv
    pfr = mean / 2.0
    maf = pfr if pfr < 1.0 - pfr else 1.0 - pfr
    if maf < qc.min_snp_maf:
        return 3
    if abs(pfr) < 1e-9 or abs(1.0 - pfr) < 1e-9:
        return 4
    if qc.max_snp_hwe_p_value < 1.0 and hwe(n0, n1, n2) <= qc.max_snp_hwe_p_value:
        return 5
    var = 0.0
    if nv >= 2:
        num = float(nv) * float(s2) - float(s1) * float(s1)              # exact: integers below 2^53
        var = (num / float(nv)) / float(nv - 1)
    return 6 if var <= 1e-9 else 0


Expected = namedtuple("Expected", "keep reason mu sigma near")


class Case:
    """one matrix and everything the device must return for it"""

    def __init__(self, G):
        self.G = np.ascontiguousarray(G, np.int8)
        self.M, self.N = self.G.shape
        valid = self.G != MISSING
        g = np.where(valid, self.G, 0).astype(np.int64)
        self.nv, self.s1, self.s2 = valid.sum(axis=1), g.sum(axis=1), (g * g).sum(axis=1)
        self.n012 = [(self.G == v).sum(axis=1) for v in (0, 1, 2)]
        self.counts = np.stack([self.nv] + self.n012, axis=1).astype(np.uint32)
        self._exp = {}

    @functools.cached_property
    def exact(self):
        """(mu, sigma) f32 of every row with a valid call: oracle.snp_sigma_exact (exact rationals, rounded once)"""
        from oracle import oracle as O
        mu, sg = np.zeros(self.M, np.float32), np.zeros(self.M, np.float32)
        for i in np.nonzero(self.nv > 0)[0]:
            m, s = O.snp_sigma_exact(self.G[i].tolist())
            mu[i], sg[i] = np.float32(m), np.float32(s)
            assert np.float32(float(Fraction(int(self.s1[i]), int(self.nv[i])))) == mu[i]
        return mu, sg

    @functools.cached_property
    def hwe(self):
        """(chi, p) per row: p from oracle.hwe_p, chi from the restatement (for the margin)"""
        O = _oracle()
        out = []
        for i in range(self.M):
            n0, n1, n2 = (int(c[i]) for c in self.n012)
            out.append((hwe_chi_p(n0, n1, n2)[0], O.hwe_p(n0, n1, n2)))
        return out

    def expected(self, qc):
        key = (qc.min_snp_call_rate, qc.min_snp_maf, qc.max_snp_hwe_p_value)
        if key not in self._exp:
            reason, near = np.zeros(self.M, np.uint8), np.zeros(self.M, bool)
            for i in range(self.M):
                def hwe(n0, n1, n2, i=i):
                    chi, p = self.hwe[i]
                    near[i] = not clear_of(qc.max_snp_hwe_p_value, p, chi, self.N)
                    return p
                reason[i] = qc_reason(int(self.nv[i]), *(int(c[i]) for c in self.n012), int(self.s1[i]), int(self.s2[i]), self.N, qc, hwe)
            keep = (reason == 0).astype(np.uint8)
            mu, sg = self.exact
            z = np.float32(0)
            self._exp[key] = Expected(keep, reason, np.where(keep == 1, mu, z), np.where(keep == 1, sg, z), near)
        return self._exp[key]


def plant(G, kind, rng):
    """one planted row of make_matrix, in place"""
    N = G.shape[0]
    full = rng.integers(0, 3, N).astype(np.int8)
    if kind == 0: G[:] = 0
    elif kind == 1: G[:] = 2
    elif kind == 2: G[:] = MISSING
    elif kind == 3: G[:] = MISSING; G[N // 2] = 1                                   # nv == 1
    elif kind == 4: G[:] = MISSING; G[0] = 0; G[N - 1] = 2                          # two valid calls (one where N == 1)
    elif kind == 5: G[:] = np.where(np.arange(N) % 2 == 0, 0, 2)
    elif kind == 6: G[:] = 1
    elif kind == 7: G[:] = full; G[N - 1] = MISSING
    elif kind == 8: G[:] = full; G[0] = MISSING


N_PLANTS = 9


@functools.lru_cache(maxsize=None)
def sweep_case(M, N):
    return Case(make_matrix(M, N))


def make_matrix(M, N):
    rng = np.random.default_rng([20250, M, N])
    p = np.exp(rng.uniform(np.log(1.0 / (2 * N)), np.log(0.5), M))
    G = rng.binomial(2, np.broadcast_to(p[:, None], (M, N))).astype(np.int8)
    G[rng.random((M, N)) < 0.03] = MISSING
    if N in PITCH_I8 + PITCH_2B:
        T = 16 if N in PITCH_I8 else 64
        G[:, N - T:] = np.where(rng.random((M, T)) < 0.75, 2, MISSING)
    if M >= 12:
        for k in range(N_PLANTS):
            plant(G[2 + k], k, rng)
    else:
        for j in range(M // 2):
            plant(G[M - 1 - j], (M + j) % N_PLANTS, rng)
    return G


def sweep_shapes():
    return [(M_SWEEP, n) for n in N_BOTH + N_2BIT] + [(m, n) for n in N_FOR_ROWS for m in M_SMALL]


# ---------------------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------------------
def engine(store):
    return gpca.GpcaEngine(precision=_lib.PREC_I8_EXACT, storage=STORES[store] if isinstance(store, str) else store)


def device_stats(e, qc):
    st = e.snp_stats(qc)
    counts, reason = e.snp_qc_detail()
    n = e.num_pca_snps()
    return dict(mu=st["mu"], sigma=st["sigma"], keep=st["keep"], counts=counts, reason=reason, n=n,
                rows=e.pca_snp_rows() if n else np.empty(0, np.int64))


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def assert_stats(dev, case, qc, what):
    exp = case.expected(qc)
    ok = ~exp.near
    bad = lambda a, b: f"{what} {qc}: rows {np.nonzero(np.atleast_1d(a != b).reshape(len(a), -1).any(axis=1))[0][:8]}"
    assert np.array_equal(dev["counts"], case.counts), "counts, " + bad(dev["counts"], case.counts)
    assert np.array_equal(dev["reason"][ok], exp.reason[ok]), "reason, " + bad(dev["reason"], exp.reason)
    assert np.array_equal(dev["keep"][ok], exp.keep[ok]), "keep, " + bad(dev["keep"], exp.keep)
    assert np.array_equal(bits(dev["mu"])[ok], bits(exp.mu)[ok]), "mu, " + bad(bits(dev["mu"]), bits(exp.mu))
    assert np.array_equal(bits(dev["sigma"])[ok], bits(exp.sigma)[ok]), "sigma, " + bad(bits(dev["sigma"]), bits(exp.sigma))
    if ok.all():
        assert dev["n"] == int(exp.keep.sum()), what
        assert np.array_equal(dev["rows"], np.nonzero(exp.keep)[0]), what


def check_handle(e, case, what, resident=True):
    """the handle holds `case`: same download (where resident), same statistics under the three QC configurations; returns them"""
    if resident:
        assert e.dims() == (case.M, case.N)
        assert np.array_equal(e.download_genotypes_i8(), case.G), what + ": download"
    out = []
    for qc in QCS:
        out.append(device_stats(e, qc))
        assert_stats(out[-1], case, qc, what)
    return out


def assert_same_bits(a, b, what):
    for x, y in zip(a, b):
        for k in ("counts", "reason", "keep", "rows"):
            assert np.array_equal(x[k], y[k]), f"{what}: int8 and 2-bit differ in {k}"
        for k in ("mu", "sigma"):
            assert np.array_equal(bits(x[k]), bits(y[k])), f"{what}: int8 and 2-bit differ in {k}"


def encode_bed(G):
    """int8 dosages (count of A1; -127 missing) -> PLINK .bed rows; the pad fields of the last byte alternate 00 (dosage 2) and 01
    (missing), which a decoder must not let through"""
    code = np.full(G.shape, 1, np.uint8)
    code[G == 2] = 0; code[G == 1] = 2; code[G == 0] = 3
    M, N = G.shape
    pad = np.tile(np.array([0, 1, 0], np.uint8), (M, 1))[:, :(-N) % 4]
    c = np.concatenate([code, pad], axis=1).reshape(M, -1, 4)
    return np.ascontiguousarray((c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)).astype(np.uint8))


def wide_slice(G):
    """G as a column slice of a wider array whose other columns hold missing calls and 2s"""
    M, N = G.shape
    W = np.where(np.arange(N + 37)[None, :] % 2 == 0, MISSING, 2).astype(np.int8).repeat(M, axis=0)
    W[:, 5:5 + N] = G
    return W[:, 5:5 + N]


PRODUCERS = {
    "upload": lambda e, G, bed: e.upload_genotypes_i8(G),
    "upload strided": lambda e, G, bed: e.upload_genotypes_i8(wide_slice(G)),
    "upload_bed2bit": lambda e, G, bed: e.upload_bed2bit(bed, G.shape[1]),
    "host_i8": lambda e, G, bed: e.load_from_source(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), *G.shape),
    "host_bed": lambda e, G, bed: e.load_from_source(gpca.PanelSource.host_bed(lambda r0, r: bed[r0:r0 + r]), *G.shape),
    "mapped_i8": lambda e, G, bed: e.load_from_source(gpca.PanelSource.mapped_i8(G), *G.shape),
    "mapped_bed": lambda e, G, bed: e.load_from_source(gpca.PanelSource.mapped_bed(bed), *G.shape),
}


def open_stream(e, G):
    e.stream_open(gpca.PanelSource.host_i8(lambda r0, r: G[r0:r0 + r]), G.shape[0], G.shape[1], panel_rows=1, ring_slots=2, fused=False)
    info = e.stream_info()
    assert info["panel_rows"] == PANEL_ROWS and info["n_panels"] == -(-G.shape[0] // PANEL_ROWS) and G.shape[0] % PANEL_ROWS


@pytest.fixture(scope="module")
def engines():
    es = {s: engine(s) for s in STORES}
    yield es
    for e in es.values():
        e.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# A. the sweep
# ---------------------------------------------------------------------------------------------------------------------------------
def _sweep(engines, M, N):
    case = sweep_case(M, N)
    res = {}
    for s in (("int8", "2bit") if N in N_BOTH else ("2bit",)):
        engines[s].upload_genotypes_i8(case.G)
        res[s] = check_handle(engines[s], case, f"{s} {M} x {N}")
    if len(res) == 2:
        assert_same_bits(res["int8"], res["2bit"], f"{M} x {N}")


@pytest.mark.gpu
@pytest.mark.parametrize("N", N_BOTH + N_2BIT)
def test_sample_count_edges(engines, N):
    _sweep(engines, M_SWEEP, N)


@pytest.mark.gpu
@pytest.mark.parametrize("N", N_FOR_ROWS)
@pytest.mark.parametrize("M", M_SMALL)
def test_row_count_edges(engines, M, N):
    _sweep(engines, M, N)


# ---------------------------------------------------------------------------------------------------------------------------------
# B. producers
# ---------------------------------------------------------------------------------------------------------------------------------
def _producers(e, case, store, what, only_none=False):
    bed = encode_bed(case.G)
    for name, load in PRODUCERS.items():
        load(e, case.G, bed)
        if only_none:
            assert np.array_equal(e.download_genotypes_i8(), case.G), f"{what} {name}: download"
            assert_stats(device_stats(e, QCS[0]), case, QCS[0], f"{what} {name}")
        else:
            check_handle(e, case, f"{what} {name}")


@pytest.mark.gpu
@pytest.mark.parametrize("store,N", [(s, n) for s in STORES for n in N_PRODUCERS + ([3072] if s == "2bit" else [])])
def test_every_producer_at_the_edges(engines, store, N):
    case = sweep_case(M_SWEEP, N)
    _producers(engines[store], case, store, f"{store} N = {N}")
    with engine(store) as e:
        open_stream(e, case.G)
        check_handle(e, case, f"{store} N = {N} streamed", resident=False)


@pytest.mark.gpu
@pytest.mark.parametrize("store", list(STORES))
def test_producers_on_recycled_device_memory(store):
    """a check, not a provocation: one pass, every handle fresh, after a handle of the same byte size that held missing calls only"""
    with engine(store) as d:
        d.upload_genotypes_i8(np.full((M_SWEEP, 1280), MISSING, np.int8))
        d.snp_stats(QCS[0])
        assert np.array_equal(d.snp_qc_detail()[0], np.zeros((M_SWEEP, 4), np.uint32))
    for N in (1025, 5):
        case = sweep_case(M_SWEEP, N)
        bed = encode_bed(case.G)
        for name, load in PRODUCERS.items():
            with engine(store) as e:
                load(e, case.G, bed)
                assert np.array_equal(e.download_genotypes_i8(), case.G), f"{store} {name} N = {N}: download"
                assert_stats(device_stats(e, QCS[0]), case, QCS[0], f"{store} {name} N = {N} on recycled memory")
        with engine(store) as e:
            open_stream(e, case.G)
            assert_stats(device_stats(e, QCS[0]), case, QCS[0], f"{store} streamed N = {N} on recycled memory")


# ---------------------------------------------------------------------------------------------------------------------------------
# C. the device HWE p
# ---------------------------------------------------------------------------------------------------------------------------------
HWE_N = 64
HWE_LEVELS = 140
HweGrid = namedtuple("HweGrid", "triples p chi thresholds G")
EXACT_HWE = [(16, 32, 16), (9, 30, 25), (25, 30, 9), (4, 24, 36), (36, 24, 4), (1, 14, 49), (49, 14, 1)]
# the companion at 256 samples: p == 0 exactly (chi >= 100), p == 1 exactly, and p around 0.1
ZERO_N = 256
ZERO_TRIPLES = [(128, 0, 128), (100, 0, 156), (120, 10, 126), (110, 30, 110), (90, 40, 120), (64, 128, 64), (40, 112, 104), (70, 116, 70),
                (60, 140, 56)]


def all_triples(lo, hi):
    return [(n0, n1, nv - n0 - n1) for nv in range(lo, hi + 1) for n1 in range(nv + 1) for n0 in range(nv - n1 + 1)]


def lay_out(triples, N, rng):
    G = np.full((len(triples), N), MISSING, np.int8)
    for i, (n0, n1, n2) in enumerate(triples):
        row = np.full(N, MISSING, np.int8)
        row[:n0 + n1 + n2] = np.repeat(np.array([0, 1, 2], np.int8), (n0, n1, n2))
        G[i] = rng.permutation(row)
    return G


@functools.lru_cache(maxsize=None)
def hwe_grid():
    O = _oracle()
    cand = []
    for t in all_triples(HWE_N - 3, HWE_N):
        if sum(x > 0 for x in t) >= 2:                             # one class only: reason 4 or 6 whatever p is
            cand.append((O.hwe_p(*t), hwe_chi_p(*t)[0], t))
    cand.sort()
    spaced = lambda a, b: clear_of(math.sqrt(a[0] * b[0]), a[0], a[1], HWE_N) and clear_of(math.sqrt(a[0] * b[0]), b[0], b[1], HWE_N)
    rest = [c for c in cand if 0.0 < c[0] < 1.0]
    kept = [rest[0]]
    for c in rest[1:]:
        if spaced(kept[-1], c):
            kept.append(c)
    one = (1.0, 0.0, EXACT_HWE[0])
    while not spaced(kept[-1], one):
        kept.pop()
    pick = np.unique(np.round(np.linspace(0, len(kept) - 1, HWE_LEVELS)).astype(int))
    levels = [kept[i] for i in pick]
    thresholds = [math.sqrt(a[0] * b[0]) for a, b in zip(levels, levels[1:] + [one])]
    rows = levels + [(1.0, 0.0, t) for t in EXACT_HWE]
    rng = np.random.default_rng(64)
    rows = [rows[i] for i in rng.permutation(len(rows))]
    triples = [r[2] for r in rows]
    return HweGrid(triples, np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), thresholds, lay_out(triples, HWE_N, rng))


def _hwe_run(e, G, p, thresholds, what):
    e.upload_genotypes_i8(G)
    for t in thresholds:
        st = e.snp_stats(gpca.QcConfig(0.0, 0.0, t))
        reason = e.snp_qc_detail()[1]
        want = np.where((p == 0.0) if t == 0.0 else (p < t) & (t < 1.0), 5, 0).astype(np.uint8)
        assert np.array_equal(reason, want), f"{what} t = {t!r}: rows {np.nonzero(reason != want)[0]} carry {reason[reason != want]}"
        assert np.array_equal(st["keep"], (want == 0).astype(np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("store", list(STORES))
def test_device_hwe_p_by_rank_between_thresholds(engines, store):
    g = hwe_grid()
    _hwe_run(engines[store], g.G, g.p, [0.0] + g.thresholds + [1.0], store)


@pytest.mark.gpu
@pytest.mark.parametrize("store", list(STORES))
def test_device_hwe_p_is_zero_where_erf_saturates(engines, store):
    O = _oracle()
    p = np.array([O.hwe_p(*t) for t in ZERO_TRIPLES])
    G = lay_out(ZERO_TRIPLES, ZERO_N, np.random.default_rng(256))
    _hwe_run(engines[store], G, p, [0.0, 1e-6, 1.0], f"{store} N = {ZERO_N}")


def test_hwe_restatement_equals_the_oracle():
    O = _oracle()
    triples = all_triples(HWE_N - 3, HWE_N) + ZERO_TRIPLES + [(0, 0, 0), (0, 5, 0), (7, 0, 0), (0, 0, 3), (1, 0, 10 ** 9 - 1), (3, 0, 2 * 10 ** 9)]
    assert len(triples) > 8194
    for t in triples:
        assert hwe_chi_p(*t)[1] == O.hwe_p(*t), t
        assert gpca.GpcaEngine.hwe_chi_squared_p_value(*t) == O.hwe_p(*t), t       # the host copy in libgpca.so


def test_hwe_grid_is_separated():
    g = hwe_grid()
    O = _oracle()
    K = len(g.triples)
    assert 140 <= K <= 160 and len(set(g.triples)) == K
    assert all(HWE_N - 3 <= sum(t) <= HWE_N for t in g.triples) and {HWE_N - sum(t) for t in g.triples} == {0, 1, 2, 3}
    assert np.array_equal(g.p, [O.hwe_p(*t) for t in g.triples])
    assert np.array_equal((g.G != MISSING).sum(axis=1), [sum(t) for t in g.triples])
    assert all(np.array_equal([(row == v).sum() for v in (0, 1, 2)], t) for row, t in zip(g.G, g.triples))
    # every row is decided by the HWE step alone: no other reason of the chain applies at any threshold
    for row in Case(g.G).expected(gpca.QcConfig(0.0, 0.0, 1.0)).reason:
        assert row == 0
    # every threshold is 1000 margins and twice the first-order bound away from EVERY row's p: no row is skipped
    ts = g.thresholds
    assert len(ts) >= 130 and all(a < b for a, b in zip(ts, ts[1:])) and ts[0] < 1e-9 and ts[-1] > 0.9
    for t in ts:
        for p, chi in zip(g.p, g.chi):
            assert clear_of(t, p, chi, HWE_N), (t, p, chi)
    assert sorted(np.unique(g.p))[-1] == 1.0 and int((g.p == 1.0).sum()) == len(EXACT_HWE)
    for a, b in zip(ts, ts[1:]):                                   # one p level between neighbouring thresholds: rank is pinned
        assert len(np.unique(g.p[(g.p > a) & (g.p < b)])) == 1
    # p == 0 cannot be had at 64 samples ...
    chis = [hwe_chi_p(*t)[0] for t in all_triples(HWE_N - 3, HWE_N)]
    assert max(c for c in chis if c is not None) <= 64.0 and min(O.hwe_p(*t) for t in all_triples(HWE_N - 3, HWE_N)) > 1e-15
    # ... the companion has it: chi >= 100 saturates any erf within 5 ulp?  erfc(sqrt(50)) = 1.5e-23, far below one ulp of 1
    pz = [O.hwe_p(*t) for t in ZERO_TRIPLES]
    cz = [hwe_chi_p(*t)[0] for t in ZERO_TRIPLES]
    assert all(sum(t) <= ZERO_N for t in ZERO_TRIPLES)
    assert sum(p == 0.0 for p in pz) == 5 and all(c >= 100.0 for p, c in zip(pz, cz) if p == 0.0) and math.erfc(math.sqrt(50.0)) < 1e-22
    assert sum(p == 1.0 for p in pz) == 1 and all(clear_of(1e-6, p, c, ZERO_N) for p, c in zip(pz, cz))
    assert all(r == 0 for r in Case(lay_out(ZERO_TRIPLES, ZERO_N, np.random.default_rng(256))).expected(gpca.QcConfig(0.0, 0.0, 1.0)).reason)


@pytest.mark.parametrize("mut", HWE_MUTANTS)
def test_hwe_teeth(mut):
    g = hwe_grid()
    O = _oracle()
    ts = [0.0] + g.thresholds
    kept = lambda p: [tuple(np.asarray(p) <= t if t > 0.0 else np.asarray(p) == 0.0) for t in ts]
    pm = [hwe_chi_p(*t, mut=mut)[1] for t in g.triples]
    if mut in HWE_MUTANTS_THE_GRID_REJECTS:
        assert kept(pm) != kept(g.p), mut
        return
    # the two mutants no matrix below 1e9 samples can tell apart (module docstring): equal on every triple a 64-sample row can hold ...
    for t in all_triples(HWE_N - 3, HWE_N) + ZERO_TRIPLES:
        assert hwe_chi_p(*t, mut=mut)[1] == O.hwe_p(*t), (mut, t)
    assert kept(pm) == kept(g.p)
    if mut == "no_inf_branch":                                     # ... and the removed branch shows where e1 <= 1e-9 with a hom1 call
        t = (1, 0, 10 ** 9 - 1)
        assert O.hwe_p(*t) == 0.0 and hwe_chi_p(*t)[1] == 0.0 and hwe_chi_p(*t, mut=mut)[1] > 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# D. every byte value
# ---------------------------------------------------------------------------------------------------------------------------------
BYTES_N = 67


def byte_position(v, j):
    if v % 2 == 1 and j == 0:
        return 0
    if v % 2 == 1 and j == 2:
        return BYTES_N - 1
    q, w = v % 4, (v >> 2) % 4
    return 16 * q + 4 * w + j


@functools.lru_cache(maxsize=None)
def byte_case():
    rng = np.random.default_rng(67)
    G = rng.integers(0, 3, (1024, BYTES_N)).astype(np.int8)
    G[rng.random(G.shape) < 0.03] = MISSING
    for v in range(256):
        for j in range(4):
            G[4 * v + j, byte_position(v, j)] = np.uint8(v).astype(np.int8)
    return Case(G)


def as_missing(G):
    """what explicit 2-bit storage holds: every byte outside {0, 1, 2} is a missing call"""
    return np.where((G >= 0) & (G <= 2), G, MISSING).astype(np.int8)


def _refused(e):
    with pytest.raises(gpca.GpcaError) as err:
        e.rsvd(2, 2, 1, 1)
    assert err.value.status in (-5, -9)


@pytest.mark.gpu
def test_every_byte_value_int8(engines):
    case = byte_case()
    e = engines["int8"]
    e.upload_genotypes_i8(case.G)
    assert np.array_equal(e.download_genotypes_i8(), case.G)
    assert_stats(device_stats(e, QCS[0]), case, QCS[0], "every byte, int8")
    _refused(e)


@pytest.mark.gpu
def test_every_byte_value_2bit_and_auto(engines):
    case = byte_case()
    seen = Case(as_missing(case.G))
    e = engines["2bit"]
    e.upload_genotypes_i8(case.G)
    assert np.array_equal(e.download_genotypes_i8(), seen.G)
    assert_stats(device_stats(e, QCS[0]), seen, QCS[0], "every byte, 2-bit")
    _refused(e)
    G = sweep_case(M_SWEEP, 1024).G.copy()
    G[77, 1023] = 3
    with gpca.GpcaEngine(precision=_lib.PREC_DEFAULT, storage=_lib.STORE_AUTO) as a:
        a.upload_genotypes_i8(sweep_case(M_SWEEP, 1024).G)
        assert a.storage_in_use()[0] == _lib.STORE_2BIT
        a.upload_genotypes_i8(G)
        assert a.storage_in_use()[0] == _lib.STORE_INT8 and np.array_equal(a.download_genotypes_i8(), G)
        assert_stats(device_stats(a, QCS[0]), Case(G), QCS[0], "one invalid byte under STORE_AUTO")
        _refused(a)


def fast_path_word(v, mask=0x7C7C7C7C, vm_clears_bit0=True, or_form=True):
    """k_snp_stats' packed-byte step on one uint32 word: (weird, nmiss, sum, sum of squares)"""
    v = int(v) & 0xFFFFFFFF
    m7 = v & 0x80808080
    nmiss = bin(m7).count("1")
    t3 = ((~v) | (v >> 1)) if or_form else ((~v) & (v >> 1))
    weird = (v & mask) | ((v & (v >> 1)) & 0x01010101) | ((m7 >> 7) & t3 & 0x01010101)
    vm = v & ~(m7 | ((m7 >> 7) if vm_clears_bit0 else 0)) & 0xFFFFFFFF
    b = np.array([(vm >> (8 * k)) & 0xFF for k in range(4)], np.uint8).astype(np.int8).astype(np.int64)      # sdot4: signed bytes
    return (weird & 0xFFFFFFFF) != 0, nmiss, int(b.sum()), int((b * b).sum())


def recount_word(bytes4):
    s = np.array(bytes4, np.uint8).astype(np.int8).astype(np.int64)
    weird = bool(np.any(~np.isin(s, (0, 1, 2, MISSING))))
    ok = s[s != MISSING]
    return weird, int((s == MISSING).sum()), int(ok.sum()), int((ok * ok).sum())


FILLERS = [(0, 0, 0), (0, 1, 2), (0x81, 0x81, 0x81), (2, 0x81, 1), (2, 2, 2)]
WORD_MUTANTS = {"mask off by one bit": dict(mask=0x7C7C7C78), "m7 >> 7 dropped": dict(vm_clears_bit0=False), "and for or": dict(or_form=False)}


def _word_disagreements(**mut):
    bad = set()
    for v in range(256):
        for j in range(4):
            for f in FILLERS:
                b = list(f); b.insert(j, v)
                got, want = fast_path_word(sum(x << (8 * k) for k, x in enumerate(b)), **mut), recount_word(b)
                if got[0] != want[0] or (not want[0] and got != want):
                    bad.add(v)
    return bad


def test_fast_path_restatement_classifies_every_byte_value():
    assert _word_disagreements() == set()


@pytest.mark.parametrize("name", list(WORD_MUTANTS))
def test_fast_path_teeth(name):
    assert _word_disagreements(**WORD_MUTANTS[name]), name


def test_byte_matrix_covers_every_lane_and_both_ends():
    case = byte_case()
    pos = {(v, j): byte_position(v, j) for v in range(256) for j in range(4)}
    assert all(0 <= p < BYTES_N and p % 4 == j for (v, j), p in pos.items())
    assert all(case.G[4 * v + j, p] == np.uint8(v).astype(np.int8) for (v, j), p in pos.items())
    assert {v for (v, j), p in pos.items() if p == 0} >= set(range(1, 256, 2)) and {v for (v, j), p in pos.items() if p == BYTES_N - 1} >= set(range(1, 256, 2))
    assert len({p // 16 for p in pos.values()}) == 5 and len({(p // 4) % 4 for p in pos.values()}) == 4
    valid_rows = [4 * v + j for v in (0, 1, 2, 0x81) for j in range(4)]
    assert np.all(np.isin(case.G[valid_rows], (0, 1, 2, MISSING)))
    assert all(np.any(~np.isin(case.G[4 * v + j], (0, 1, 2, MISSING))) for v in range(256) if v not in (0, 1, 2, 0x81) for j in range(4))


# ---------------------------------------------------------------------------------------------------------------------------------
# E. decisions at equality
# ---------------------------------------------------------------------------------------------------------------------------------
def _row(N, twos=0, ones=0, missing=0):
    r = np.zeros(N, np.int8)
    r[:twos] = 2; r[twos:twos + ones] = 1
    if missing:
        r[N - missing:] = MISSING
    return r


MAF_HI = 1.0 - (38 / 20) / 2.0                 # 1 - pfr of 38 alt alleles in 20 calls, as f64 evaluates it: 0.05000000000000004
EQ_CASES = {
    # name: (matrix, [(qc, {row: reason})])
    "call rate 49 / 50": (np.stack([_row(50, 3, 5, 1), _row(50, 3, 5, 2)]), [(gpca.QcConfig(0.98, 0.0, 1.0), {0: 0, 1: 1})]),
    "call rate 9 / 10": (np.stack([_row(10, 1, 2, 1), _row(10, 1, 2, 2), _row(10, 1, 2, 0)]), [(gpca.QcConfig(0.9, 0.0, 1.0), {0: 0, 1: 1, 2: 0})]),
    "maf and order": (np.stack([_row(20, 1, 0), _row(20, 0, 1), _row(20, 18, 2), _row(20, 19, 1), _row(20, 20, 0),          # 0..4
                                np.where(np.arange(20) == 7, 1, MISSING).astype(np.int8),                                # 5: nv == 1
                                np.where(np.arange(20) % 19 == 0, 0, MISSING).astype(np.int8),                           # 6: two calls 0, 0
                                np.where(np.arange(20) % 19 == 0, 2, MISSING).astype(np.int8),                           # 7: 2, 2
                                np.where(np.arange(20) % 19 == 0, 1, MISSING).astype(np.int8)]),                         # 8: 1, 1
                      [(gpca.QcConfig(0.0, 0.05, 1.0), {0: 0, 1: 3, 2: 0, 3: 3, 4: 3, 5: 6, 6: 3, 7: 3, 8: 6}),
                       (gpca.QcConfig(0.0, MAF_HI, 1.0), {2: 0, 3: 3, 0: 3}),
                       (gpca.QcConfig(0.0, 0.0, 1.0), {4: 4, 5: 6, 6: 4, 7: 4, 8: 6, 0: 0, 2: 0})]),
}


def test_equality_rows_sit_exactly_on_their_thresholds():
    assert 49 / 50 == 0.98 and 9 / 10 == 0.9 and (2 / 20) / 2.0 == 0.05 and MAF_HI != 0.05 and 0.05 < MAF_HI < 0.05 + 1e-16
    for name, (G, runs) in EQ_CASES.items():
        case = Case(G)
        for qc, pinned in runs:
            exp = case.expected(qc)
            assert not exp.near.any()
            for row, reason in pinned.items():
                assert exp.reason[row] == reason, (name, qc, row)
    G = EQ_CASES["maf and order"][0]
    c = Case(G)
    assert c.s1[0] / c.nv[0] / 2.0 == 0.05 and 1.0 - c.s1[2] / c.nv[2] / 2.0 == MAF_HI and c.nv[5] == 1 and c.nv[6] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("store", list(STORES))
@pytest.mark.parametrize("name", list(EQ_CASES))
def test_decisions_at_equality(engines, store, name):
    G, runs = EQ_CASES[name]
    case = Case(G)
    engines[store].upload_genotypes_i8(case.G)
    for qc, _ in runs:
        assert_stats(device_stats(engines[store], qc), case, qc, f"{store} {name}")


# ---------------------------------------------------------------------------------------------------------------------------------
# F. standardize_block
# ---------------------------------------------------------------------------------------------------------------------------------
def block_request(case):
    """(PCA SNP ids, sample ids with no missing call in those rows, sample ids with one, kept rows) under QcConfig.none()"""
    N = case.N
    rows = np.nonzero(case.expected(QCS[0]).keep)[0]
    want = {0, len(rows) - 1} | {int(np.nonzero(rows % 4 == ph)[0][3]) for ph in range(4)}     # first, last, one per KiB phase
    want |= {int(k) for k in np.nonzero(np.isin(rows, (9, 10)))[0]}                           # missing in the last / the first sample
    sid = np.array(sorted(want), np.int64)[::-1].copy()                                       # not in row order
    ids = sorted({n for n in range(N) if n < 5 or n == N - 1 or n % 4 != 2 or (n + 1) % 16 == 0})
    miss = (case.G[rows[sid]] == MISSING).any(axis=0)
    clean = np.array([n for n in ids if not miss[n]], np.int64)
    dirty = np.array([n for n in range(N) if miss[n]], np.int64)
    return sid, clean, dirty, rows


def test_block_requests_cover_the_boundaries():
    for N in N_BLOCK:
        case = sweep_case(M_SWEEP, N)
        sid, clean, dirty, rows = block_request(case)
        assert {int(r) % 4 for r in rows[sid]} == {0, 1, 2, 3} and rows[sid].min() == rows[0] and rows[sid].max() == rows[-1]
        assert len(clean) >= min(N, 64) - 2 and len(dirty) >= 2 and {0, N - 1} <= set(dirty.tolist())
        if N > 16:
            assert {int(n) % 4 for n in clean} >= {0, 1, 3} and {int(n) % 16 for n in clean} >= {0, 1, 15}


@pytest.mark.gpu
@pytest.mark.parametrize("store", list(STORES))
@pytest.mark.parametrize("N", N_BLOCK)
def test_standardize_block_at_byte_and_vector_boundaries(engines, store, N):
    O = _oracle()
    case = sweep_case(M_SWEEP, N)
    e = engines[store]
    e.upload_genotypes_i8(case.G)
    st = e.snp_stats(QCS[0])
    assert_stats(device_stats(e, QCS[0]), case, QCS[0], f"{store} N = {N}")
    sid, clean, dirty, rows = block_request(case)
    ref, err = O.standardize_block(case.G, st["mu"], st["sigma"], rows[sid], clean)
    assert err is None
    out = e.standardize_block(sid, clean)
    assert np.array_equal(bits(out), bits(ref))
    for a in range(len(sid)):                                      # one row at a time, every sample that row has a call for
        cols = np.nonzero(case.G[rows[sid[a]]] != MISSING)[0]
        ref, err = O.standardize_block(case.G, st["mu"], st["sigma"], rows[sid[a:a + 1]], cols)
        assert err is None and np.array_equal(bits(e.standardize_block(sid[a:a + 1], cols)), bits(ref))
    cols = np.concatenate([clean[:3], dirty[::-1], clean[3:]])      # missing calls in the middle of the request, several of them
    _, err = O.standardize_block(case.G, st["mu"], st["sigma"], rows[sid], cols)
    assert err is not None
    with pytest.raises(gpca.GpcaError) as ex:
        e.standardize_block(sid, cols)
    assert ex.value.status == -5
    a, c = err
    assert f"for PCA SNP ID {sid[a]} (original BIM index {rows[sid[a]]}), requested sample index {cols[c]}." in ex.value.message


# ---------------------------------------------------------------------------------------------------------------------------------
# the model against the oracle, and the inputs' own conditions (CPU)
# ---------------------------------------------------------------------------------------------------------------------------------
def every_case():
    yield from ((f"sweep {m} x {n}", sweep_case(m, n)) for m, n in sweep_shapes())
    yield "every byte", byte_case()
    yield "every byte as 2-bit codes", Case(as_missing(byte_case().G))
    yield from ((name, Case(G)) for name, (G, _) in EQ_CASES.items())
    yield "hwe grid", Case(hwe_grid().G)


def test_chain_restatement_equals_the_oracle():
    """qc_reason, the counts and mu against oracle.snp_stats (two-pass f64) on every matrix of the module; sigma within the f32 ulp the
    two-pass sum may lose, and equal to it on all but a few rows"""
    O = _oracle()
    qcs = list(QCS) + [qc for _, runs in EQ_CASES.values() for qc, _ in runs]
    for name, case in every_case():
        for qc in qcs:
            ref = O.snp_stats(case.G, case.N, qc.min_snp_call_rate, qc.min_snp_maf, qc.max_snp_hwe_p_value)
            exp = case.expected(qc)
            assert np.array_equal(ref["counts"], case.counts), name
            assert np.array_equal(ref["reason"], exp.reason), (name, qc, np.nonzero(ref["reason"] != exp.reason)[0])
            assert np.array_equal(ref["keep"], exp.keep) and np.array_equal(bits(ref["mu"]), bits(exp.mu)), (name, qc)
            assert np.all(np.abs(ref["sigma"].astype(np.float64) - exp.sigma.astype(np.float64)) <= np.spacing(ref["sigma"])), (name, qc)


def test_no_sweep_row_stands_near_an_hwe_threshold():
    """the carve-out of section A is empty: the seeds leave no row within the margin of 1e-6 or 1e-3"""
    for name, case in every_case():
        for qc in QCS:
            assert not case.expected(qc).near.any(), (name, qc, np.nonzero(case.expected(qc).near)[0])


def test_sweep_inputs_hold_what_the_docstring_says():
    for N in PITCH_I8 + PITCH_2B:
        G = sweep_case(M_SWEEP, N).G
        T = 16 if N in PITCH_I8 else 64
        dense = np.ones(M_SWEEP, bool); dense[2:2 + N_PLANTS] = False
        assert np.all(np.isin(G[dense, N - T:], (2, MISSING))) and np.all((G[dense, N - T:] == 2).sum(axis=1) >= 4)
    for N in N_BOTH + N_2BIT:
        case = sweep_case(M_SWEEP, N)
        G = case.G
        assert np.all(G[2] == 0) and np.all(G[3] == 2) and np.all(G[4] == MISSING) and case.nv[5] == 1 and case.nv[6] == min(N, 2)
        assert np.all(G[8] == 1) and G[9, -1] == MISSING and G[10, 0] == MISSING and case.nv[9] == N - 1 and case.nv[10] == N - 1
        if N >= 64:                                                # every reason of the chain occurs somewhere in the three runs
            seen = set()
            for qc in QCS:
                seen |= set(case.expected(qc).reason.tolist())
            assert seen >= {0, 1, 2, 3, 4, 6}, (N, seen)
    assert any(5 in sweep_case(M_SWEEP, N).expected(QCS[2]).reason for N in N_BOTH)
