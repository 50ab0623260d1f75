"""CPU-only: the host rules of include/gpca.h section a17 (gpca_fst_hudson, gpca_fst_wc) and the readers and writers around them
(io.read_within, io.align_within, io.group_count_bands, io.write_frq_strat, io.write_fst_summary, io.write_fst_var and their twins in
host/formats.hpp).

``hudson_restate`` and ``wc_restate`` restate the header's evaluation order in Python floats (IEEE f64, one operation at a time, so no
fused multiply-add): the library is held to them at rtol 1e-13 (the order is the same, so the bits are expected to agree).  The NaN and
contribution rules are checked at n_obs in {0, 1, 2} and on a SNP fixed in both groups; sums over bands against one call bit for bit.
What it is for: three Balding-Nichols populations with F = 0.1 (sizes 60 / 100 / 37, 20 000 SNPs, 2 % missing) give Hudson and
Weir-Cockerham values within 0.01 of 0.1 -- the per-SNP ratio scatters by about 0.15, so the ratio of sums over 20 000 SNPs has a
standard error near 0.001, and the finite-sample bias of either estimator at these sizes is below 0.003."""
import os
import subprocess

import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import _lib
from genomic_pca_amd import io as gio
from genomic_pca_amd._lib import GpcaError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


# ------------------------------------------------------------------------------------------------ the header's order
def _freq(c):
    n = 2.0 * float(c[0])
    return n, (float(c[1]) + 2.0 * float(c[2])) / n


def hudson_restate(counts):
    rows, P = counts.shape[:2]
    pairs = P * (P - 1) // 2
    num, den, sums = np.full((rows, pairs), NAN), np.full((rows, pairs), NAN), np.zeros((pairs, 3))
    for r in range(rows):
        for i in range(1, P):
            for j in range(i):
                q = i * (i - 1) // 2 + j
                ci, cj = counts[r, i], counts[r, j]
                if ci[0] >= 1 and cj[0] >= 1:
                    ni, pi = _freq(ci)
                    nj, pj = _freq(cj)
                    d = pi - pj
                    nu = (d * d - (pi * (1.0 - pi)) / (ni - 1.0)) - (pj * (1.0 - pj)) / (nj - 1.0)
                    de = pi * (1.0 - pj) + pj * (1.0 - pi)
                    num[r, q], den[r, q] = nu, de
                    sums[q, 0] += nu; sums[q, 1] += de; sums[q, 2] += 1.0
    return num, den, sums


def wc_restate(counts, use=None):
    rows, P = counts.shape[:2]
    used = [p for p in range(P) if use is None or use[p]]
    r_ = float(len(used))
    abc, sums = np.full((rows, 3), NAN), np.zeros(3)
    for i in range(rows):
        c = counts[i]
        nt = sq = 0.0
        ok = True
        for p in used:
            n = float(c[p, 0])
            ok = ok and c[p, 0] >= 1
            nt += n; sq += n * n
        if not ok or not nt > r_:
            continue
        sp = sh = 0.0
        for p in used:
            n = float(c[p, 0])
            sp += n * _freq(c[p])[1]
            sh += n * (float(c[p, 1]) / n)
        nbar, nc, pbar, hbar = nt / r_, (nt - sq / nt) / (r_ - 1.0), sp / nt, sh / nt
        ss = 0.0
        for p in used:
            d = _freq(c[p])[1] - pbar
            ss += float(c[p, 0]) * (d * d)
        s2 = ss / ((r_ - 1.0) * nbar)
        core = pbar * (1.0 - pbar) - ((r_ - 1.0) / r_) * s2
        a = (nbar / nc) * (s2 - (core - hbar / 4.0) / (nbar - 1.0))
        b = (nbar / (nbar - 1.0)) * (core - ((2.0 * nbar - 1.0) / (4.0 * nbar)) * hbar)
        cc = hbar / 2.0
        abc[i] = a, b, cc
        sums[0] += a; sums[1] += (a + b) + cc; sums[2] += 1.0
    return abc, sums


def random_counts(rows, P, seed, nmax=40):
    rng = np.random.default_rng(seed)
    obs = rng.integers(0, nmax, (rows, P))
    obs[rows // 3, 0] = 0                                   # (a group without an observed call, whatever the draw)
    het = (rng.random((rows, P)) * (obs + 1)).astype(np.int64)
    hom = (rng.random((rows, P)) * (obs - het + 1)).astype(np.int64)
    return np.stack([obs, het, hom], -1).astype(np.uint32)


def close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.allclose(a[~np.isnan(a)], b[~np.isnan(b)], rtol=1e-13, atol=0.0)


# ------------------------------------------------------------------------------------------------ the two rules
@pytest.mark.parametrize("P", [2, 3, 7, 64])
def test_hudson_against_the_restatement(P):
    c = random_counts(60 if P < 64 else 6, P, seed=P)
    fst, sums, num, den = gpca.fst_hudson(c, per_variant=True)
    rnum, rden, rsums = hudson_restate(c)
    assert close(num, rnum) and close(den, rden) and close(sums, rsums)
    assert np.array_equal(sums[:, 2], rsums[:, 2])
    assert close(fst, rsums[:, 0] / rsums[:, 1])
    assert np.isnan(num).any() and np.isfinite(num).any()


@pytest.mark.parametrize("P", [2, 3, 7, 64])
def test_wc_against_the_restatement(P):
    c = random_counts(60 if P < 64 else 200, P, seed=10 + P, nmax=40 if P < 64 else 400)
    if P == 64:
        c[:, :, 0] = np.maximum(c[:, :, 0], 1)             # (with 64 groups a random row would never have them all observed)
        c[:, :, 1] = np.minimum(c[:, :, 1], c[:, :, 0]); c[:, :, 2] = np.minimum(c[:, :, 2], c[:, :, 0] - c[:, :, 1])
    fst, sums, abc = gpca.fst_wc(c, per_variant=True)
    rabc, rsums = wc_restate(c)
    assert close(abc, rabc) and close(sums, rsums) and sums[2] == rsums[2] and sums[2] > 0
    assert close(fst, rsums[0] / rsums[1])


def test_the_use_mask():
    c = random_counts(80, 5, seed=21)
    use = np.array([1, 0, 1, 1, 0], np.uint8)
    fst, sums, abc = gpca.fst_wc(c, use=use, per_variant=True)
    rabc, rsums = wc_restate(c, use)
    assert close(abc, rabc) and close(sums, rsums)
    sub = np.ascontiguousarray(c[:, [0, 2, 3]])            # the same groups as a table of their own: the same bits
    fst2, sums2, abc2 = gpca.fst_wc(sub, per_variant=True)
    assert np.array_equal(abc, abc2, equal_nan=True) and np.array_equal(sums, sums2)
    # a pair through the mask is Hudson's pair's rows: both need n_obs >= 1 in both groups (and WC n_t > 2)
    pair = np.array([0, 1, 0, 1, 0], np.uint8)
    _, s2, abc_p = gpca.fst_wc(c, use=pair, per_variant=True)
    both = (c[:, 1, 0] >= 1) & (c[:, 3, 0] >= 1) & (c[:, 1, 0] + c[:, 3, 0] > 2)
    assert np.array_equal(~np.isnan(abc_p[:, 0]), both) and s2[2] == both.sum()


def test_nan_and_contribution_rules():
    # rows: n_obs of group 0 = 0, 1, 2 against a full group 1; then a SNP fixed in both groups; then both groups at one sample
    c = np.array([[[0, 0, 0], [10, 4, 3]],
                  [[1, 1, 0], [10, 4, 3]],
                  [[2, 1, 1], [10, 4, 3]],
                  [[5, 0, 5], [7, 0, 7]],
                  [[1, 0, 0], [1, 0, 1]]], np.uint32)
    fst, sums, num, den = gpca.fst_hudson(c, per_variant=True)
    assert np.isnan(num[0, 0]) and np.isnan(den[0, 0]) and np.isfinite(num[1:, 0]).all()
    assert sums[0, 2] == 4
    assert num[3, 0] == 0.0 and den[3, 0] == 0.0                                         # fixed in both: 0 / 0, yet a row used
    assert num[4, 0] == 1.0 and den[4, 0] == 1.0                                         # n = 2 alleles each: n - 1 = 1
    rnum, rden, rsums = hudson_restate(c)
    assert close(num, rnum) and close(sums, rsums)
    only = np.ascontiguousarray(c[3:4])
    f1, s1 = gpca.fst_hudson(only)
    assert np.isnan(f1[0]) and s1[0, 1] == 0.0 and s1[0, 2] == 1
    _, wsums, abc = gpca.fst_wc(c, per_variant=True)
    assert np.isnan(abc[0]).all()                                                        # a used group without an observed call
    assert np.isfinite(abc[1:4]).all()
    assert np.isnan(abc[4]).all()                                                        # n_t = 2 = r
    assert wsums[2] == 3
    assert abc[3, 0] == 0.0 and abc[3, 1] == 0.0 and abc[3, 2] == 0.0
    fw, sw = gpca.fst_wc(only)
    assert np.isnan(fw) and sw[1] == 0.0 and sw[2] == 1


def test_sums_over_bands_are_the_sums_of_one_call():
    c = random_counts(101, 4, seed=33)
    _, hs = gpca.fst_hudson(c)
    _, ws = gpca.fst_wc(c)
    for cut in (0, 1, 50, 100, 101):
        h2, w2 = np.zeros_like(hs), np.zeros(3)
        for band in (c[:cut], c[cut:]):
            gpca.fst_hudson(np.ascontiguousarray(band), sums=h2)
            gpca.fst_wc(np.ascontiguousarray(band), sums=w2)
        assert np.array_equal(h2, hs) and np.array_equal(w2, ws), cut
    three = np.zeros_like(hs)
    for band in (c[:7], c[7:64], c[64:]):
        gpca.fst_hudson(np.ascontiguousarray(band), sums=three)
    assert np.array_equal(three, hs)


def test_bad_arguments():
    import ctypes
    lib = _lib.load()
    c = random_counts(4, 3, seed=1)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    s9, s3, use1 = np.zeros(9), np.zeros(3), np.array([1, 0, 0], np.uint8)
    BA = _lib.GPCA_ERR_BAD_ARG
    assert lib.gpca_fst_hudson(vp(c), 4, 3, None, None, vp(s9)) == 0
    assert lib.gpca_fst_hudson(None, 4, 3, None, None, vp(s9)) == BA
    assert lib.gpca_fst_hudson(vp(c), 4, 3, None, None, None) == BA
    assert lib.gpca_fst_hudson(vp(c), -1, 3, None, None, vp(s9)) == BA
    for P in (1, 0, 65, -2):
        assert lib.gpca_fst_hudson(vp(c), 1, P, None, None, vp(s9)) == BA
    assert lib.gpca_fst_wc(vp(c), 4, 3, None, None, vp(s3)) == 0
    assert lib.gpca_fst_wc(None, 4, 3, None, None, vp(s3)) == BA
    assert lib.gpca_fst_wc(vp(c), 4, 3, None, None, None) == BA
    assert lib.gpca_fst_wc(vp(c), -1, 3, None, None, vp(s3)) == BA
    for P in (0, 65, -2, 1):                                                             # (P = 1: fewer than two groups)
        assert lib.gpca_fst_wc(vp(c), 1, P, None, None, vp(s3)) == BA
    assert lib.gpca_fst_wc(vp(c), 4, 3, vp(use1), None, vp(s3)) == BA                    # fewer than two groups used
    assert lib.gpca_fst_hudson(vp(c), 0, 3, None, None, vp(s9)) == 0 and lib.gpca_fst_wc(vp(c), 0, 3, None, None, vp(s3)) == 0
    with pytest.raises(GpcaError) as ei:
        gpca.fst_wc(c, use=[1, 0, 0])
    assert ei.value.status == BA
    with pytest.raises(ValueError):
        gpca.fst_hudson(c[:, :, :2])


def test_balding_nichols_populations_give_back_their_fst():
    rng = np.random.default_rng(5)
    sizes, F, M = [60, 100, 37], 0.1, 20000
    anc = rng.uniform(0.1, 0.9, M)
    counts = np.zeros((M, 3, 3), np.uint32)
    for p, n in enumerate(sizes):
        f = rng.beta(anc * (1 - F) / F, (1 - anc) * (1 - F) / F)
        g = (rng.random((M, n)) < f[:, None]).astype(np.int8) + (rng.random((M, n)) < f[:, None]).astype(np.int8)
        miss = rng.random((M, n)) < 0.02
        counts[:, p, 0] = (~miss).sum(1)
        counts[:, p, 1] = ((g == 1) & ~miss).sum(1)
        counts[:, p, 2] = ((g == 2) & ~miss).sum(1)
    fst, _ = gpca.fst_hudson(counts)
    assert np.all(np.abs(fst - F) < 0.01), fst
    joint, _ = gpca.fst_wc(counts)
    two, _ = gpca.fst_wc(counts, use=[1, 1, 0])
    assert abs(joint - F) < 0.01 and abs(two - F) < 0.01, (joint, two)


# ------------------------------------------------------------------------------------------------ readers and writers
WITHIN = """#FID IID GROUP
f1 a EUR
f1 b AFR

f2 c NA
f3 d EUR
f9 zz EAS
f4 e AFR
"""


def test_read_and_align_within(tmp_path):
    p = tmp_path / "w.txt"
    p.write_text(WITHIN)
    t = gio.read_within(str(p))
    assert t.names == ["EUR", "AFR", "EAS"] and t.groups == ["EUR", "AFR", None, "EUR", "EAS", "AFR"]
    labels, names = gio.align_within(t, ["f4", "f1", "f2", "fX", "f1", "f3"], ["e", "a", "c", "a", "b", "d"])
    assert names == ["EUR", "AFR", "EAS"] and labels.dtype == np.int32 and labels.tolist() == [1, 0, -1, -1, 1, 0]
    for text, word in (("FID IID\nf a\n", "header"), ("FID IID GRP\nf a x\n", "header"), ("", "header"), ("fid iid group\nf a x y\n", "fields"),
                       ("FID IID GROUP\nf a x\nf a y\n", "appears twice")):
        p.write_text(text)
        with pytest.raises(ValueError) as ei:
            gio.read_within(str(p))
        assert word in str(ei.value), text
    p.write_text("fid iid group\nf a x\n")
    assert gio.read_within(str(p)).names == ["x"]
    assert gio.group_count_bands(10, 3, 1 << 26) == [(0, 10)] and gio.group_count_bands(10, 2, 24) == [(0, 4), (4, 8), (8, 10)]
    assert gio.group_count_bands(3, 64, 1) == [(0, 1), (1, 2), (2, 3)] and gio.group_count_bands(0, 3) == []


def test_writers_on_hand_written_inputs(tmp_path):
    hwe = gpca.GpcaEngine.hwe_chi_squared_p_value
    counts = np.array([[[10, 4, 3], [0, 0, 0]], [[3, 0, 3], [8, 8, 0]]], np.uint32)
    path = gio.write_frq_strat(str(tmp_path / "o.frq.strat"), ["1"], [100], ["rs1"], ["A"], ["P1", "P2"], counts[:1])
    gio.write_frq_strat(path, ["X"], [2500000], ["rs2"], ["T"], ["P1", "P2"], counts[1:], append=True)
    lines = open(path).read().splitlines()
    assert lines[0] == "#CHROM\tPOS\tID\tA1\tGROUP\tOBS_CT\tA1_CT\tA1_FREQ\tHET_CT\tHOM_A1_CT\tHWE_P"
    assert lines[1] == "1\t100\trs1\tA\tP1\t10\t10\t0.5\t4\t3\t" + ("%.6g" % hwe(3, 4, 3))
    assert lines[2] == "1\t100\trs1\tA\tP2\t0\t0\tNA\t0\t0\tNA"
    assert lines[3].startswith("X\t2500000\trs2\tT\tP1\t3\t6\t1\t0\t3\t")
    assert lines[4].startswith("X\t2500000\trs2\tT\tP2\t8\t8\t0.5\t8\t0\t") and len(lines) == 5
    names = ["A", "B", "C"]
    sums = np.array([[1.0, 8.0, 5], [0.0, 0.0, 2], [3.0, 4.0, 0]])
    lines = open(gio.write_fst_summary(str(tmp_path / "h"), "hudson", names, sums)).read().splitlines()
    assert lines == ["#GROUP1\tGROUP2\tN_VAR\tHUDSON_FST", "A\tB\t5\t0.125", "A\tC\t2\tNA", "B\tC\t0\tNA"]
    lines = open(gio.write_fst_summary(str(tmp_path / "w"), "wc", names, np.vstack([sums, [[1.0, 3.0, 9]]]))).read().splitlines()
    assert lines[0] == "#GROUP1\tGROUP2\tN_VAR\tWC_FST" and lines[-1] == "*\t*\t9\t0.333333" and len(lines) == 5
    lines = open(gio.write_fst_summary(str(tmp_path / "w2"), "wc", names[:2], sums[:1])).read().splitlines()
    assert lines == ["#GROUP1\tGROUP2\tN_VAR\tWC_FST", "A\tB\t5\t0.125"]
    with pytest.raises(ValueError):
        gio.write_fst_summary(str(tmp_path / "w3"), "wc", names, sums)
    hv = np.array([[[0.01, 0.04], [NAN, NAN], [0.0, 0.0]]])
    lines = open(gio.write_fst_var(str(tmp_path / "h"), "hudson", ["1"], [100], ["rs1"], names, hv)).read().splitlines()
    assert lines == ["#CHROM\tPOS\tID\tGROUP1\tGROUP2\tNUM\tDEN\tFST", "1\t100\trs1\tA\tB\t0.01\t0.04\t0.25", "1\t100\trs1\tA\tC\tNA\tNA\tNA",
                     "1\t100\trs1\tB\tC\t0\t0\tNA"]
    wv = np.array([[[0.5, 0.25, 0.25], [NAN, NAN, NAN], [0.0, 0.0, 0.0]]])
    lines = open(gio.write_fst_var(str(tmp_path / "w"), "wc", ["1"], [100], ["rs1"], names, wv)).read().splitlines()
    assert lines == ["#CHROM\tPOS\tID\tGROUP1\tGROUP2\tA\tB\tC\tFST", "1\t100\trs1\tA\tB\t0.5\t0.25\t0.25\t0.5", "1\t100\trs1\tA\tC\tNA\tNA\tNA\tNA",
                     "1\t100\trs1\tB\tC\t0\t0\t0\tNA"]


def test_formats_hpp_writes_the_same_bytes(tmp_path):
    gpca.load()
    pkg = os.path.join(ROOT, "genomic_pca_amd")
    exe = str(tmp_path / "dump_strat")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(pkg, "host"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "dump_strat.cpp"), "-o", exe, "-L" + pkg, "-lgpca", "-lz", "-Wl,-rpath," + pkg])
    M, P = 23, 4
    names = ["EUR", "AFR", "EAS", "none"]
    c = random_counts(M, P, seed=77)
    c[:, 3] = 0                                                                          # an empty group
    c[5, 0] = (6, 0, 6); c[5, 1] = (9, 0, 9)                                             # fixed in both
    chrom, pos = [str(1 + i // 8) for i in range(M)], [1000 * (i + 1) for i in range(M)]
    ids, a1 = [f"rs{i}" for i in range(M)], ["ACGT"[i % 4] for i in range(M)]
    fam = [("f4", "e"), ("f1", "a"), ("f2", "c"), ("fX", "a"), ("f1", "b"), ("f3", "d")]
    within, data = tmp_path / "w.txt", tmp_path / "d.txt"
    within.write_text(WITHIN)
    with open(data, "w") as f:
        f.write(f"{M} {P} {len(fam)}\n" + " ".join(names) + "\n")
        for i in range(M):
            f.write(f"{chrom[i]} {pos[i]} {ids[i]} {a1[i]} " + " ".join(str(int(v)) for v in c[i].reshape(-1)) + "\n")
        f.writelines(f"{a} {b}\n" for a, b in fam)
    cpp = str(tmp_path / "cpp" / "o")
    out = subprocess.run([exe, cpp, str(within), str(data)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    t = gio.read_within(str(within))
    labels, _ = gio.align_within(t, [a for a, _ in fam], [b for _, b in fam])
    want = ["names " + " ".join(t.names), "labels " + " ".join(str(int(v)) for v in labels)]
    for mv in (1 << 26, 1000, 1):
        for p in (1, 3, 64):
            want.append(f"bands {mv} {p}:" + "".join(f" {a}-{b}" for a, b in gio.group_count_bands(1000, p, mv)))
    assert out.stdout.splitlines() == want
    # the same files through io.py, in the same two bands
    py = str(tmp_path / "py" / "o")
    pairs = gio.fst_pairs(P)
    hud, wcp, wcj = np.zeros((len(pairs), 3)), np.zeros((len(pairs), 3)), np.zeros(3)
    for bi, (r0, r1) in enumerate(((0, M // 2), (M // 2, M))):
        cb = np.ascontiguousarray(c[r0:r1])
        meta = (chrom[r0:r1], pos[r0:r1], ids[r0:r1])
        gio.write_frq_strat(py + ".frq.strat", *meta, a1[r0:r1], names, cb, append=bi > 0)
        _, _, num, den = gpca.fst_hudson(cb, sums=hud, per_variant=True)
        gio.write_fst_var(py + "_h", "hudson", *meta, names, np.stack([num, den], -1), append=bi > 0)
        abc = np.zeros((r1 - r0, len(pairs), 3))
        for q, (j, i) in enumerate(pairs):
            use = np.zeros(P, np.uint8); use[[j, i]] = 1
            abc[:, q] = gpca.fst_wc(cb, use, sums=wcp[q], per_variant=True)[2]
        gpca.fst_wc(cb, None, sums=wcj)
        gio.write_fst_var(py + "_w", "wc", *meta, names, abc, append=bi > 0)
    gio.write_fst_summary(py + "_h", "hudson", names, hud)
    gio.write_fst_summary(py + "_w", "wc", names, np.vstack([wcp, wcj[None]]))
    for suffix in (".frq.strat", "_h.fst.summary", "_h.fst.var", "_w.fst.summary", "_w.fst.var"):
        a, b = open(py + suffix, "rb").read(), open(cpp + suffix, "rb").read()
        assert a == b and len(a) > 100, suffix
    assert b"\tNA" in open(py + "_h.fst.var", "rb").read() and b"\tNA" in open(py + ".frq.strat", "rb").read()
