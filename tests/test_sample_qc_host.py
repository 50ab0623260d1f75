"""CPU-only: the two host rules of include/gpca.h section a18 (gpca_het_weights, gpca_sample_het) against a numpy restatement at rtol
1e-13 (the bar of the Fst host rules: a handful of f64 operations per value), io.sample_qc_pass and the four writers against
hand-built tables with their NaN / NA rows, and a worked example checked by the numpy model alone: 400 samples x 5 000 SNPs of one
population with two contaminated samples (mixed 50/50 with another sample's genotypes), two with excess homozygosity and three with
8 % missing calls; under mind = 0.05 and het_sd = 3 the rule flags exactly those seven."""
import numpy as np
import pytest

import genomic_pca_amd as gpca
from genomic_pca_amd import io as gio

Q30 = float(1 << 30)


def counts_model(G):
    """uint32 [N][3] = n_obs, n_het, n_hom2 per sample; uint32 [M][4] = n_valid, n_hom0, n_het, n_hom2 per row"""
    obs = G != -127
    per_sample = np.stack([obs.sum(0), (G == 1).sum(0), (G == 2).sum(0)], 1).astype(np.uint32)
    per_row = np.stack([obs.sum(1), (G == 0).sum(1), (G == 1).sum(1), (G == 2).sum(1)], 1).astype(np.uint32)
    return per_sample, per_row


def het_weights_model(qc):
    qc = np.asarray(qc, np.float64)
    t = 2.0 * qc[:, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        p = (qc[:, 2] + 2.0 * qc[:, 3]) / t
        e = ((2.0 * p) * (1.0 - p)) * (t / (t - 1.0))
    return np.where(qc[:, 0] == 0, 0.0, e)                    # the expected heterozygosity itself, before the 2^30 grid


def sample_het_model(counts, qsum):
    n = counts[:, 0].astype(np.float64)
    ohom = n - counts[:, 1].astype(np.float64)
    ehom = n - qsum.astype(np.float64) / Q30
    den = n - ehom
    with np.errstate(invalid="ignore", divide="ignore"):
        F = np.where((counts[:, 0] == 0) | ~(den > 0.0), np.nan, (ohom - ehom) / den)
    return np.stack([ohom, ehom, F], 1)


def test_het_weights_against_the_restatement():
    rng = np.random.default_rng(1)
    n = rng.integers(1, 5000, 2000)
    het = (rng.random(2000) * n).astype(np.int64)
    hom2 = (rng.random(2000) * (n - het)).astype(np.int64)
    qc = np.stack([n, n - het - hom2, het, hom2], 1).astype(np.uint32)
    qc = np.vstack([qc, [[0, 0, 0, 0], [1, 0, 1, 0], [1, 1, 0, 0], [1, 0, 0, 1], [2, 0, 2, 0], [7, 7, 0, 0], [4000000000, 1000000000, 2000000000, 1000000000]]]).astype(np.uint32)
    q = gpca.het_weights(qc)
    assert q.dtype == np.uint32 and q.shape == (len(qc),) and int(q.max()) <= 1 << 30
    e = het_weights_model(qc)
    want = np.floor(e * Q30 + 0.5)
    # the grid value: equal, or the neighbour where e 2^30 + 0.5 lies within rtol 1e-13 of an integer
    off = np.abs(q.astype(np.float64) - want)
    frac = np.abs((e * Q30 + 0.5) - np.round(e * Q30 + 0.5))
    assert np.all((off == 0) | ((off == 1) & (frac <= 1e-13 * Q30))), int(off.max())
    np.testing.assert_allclose(q / Q30, e, rtol=0, atol=0.5 / Q30 * (1 + 1e-13))
    assert q[2000] == 0 and q[2001] == 1 << 30 and q[2002] == 0 and q[2003] == 0 and q[2005] == 0      # p = 1/2 of one sample: e = 1
    assert q[2004] == int(np.floor((0.5 * (4.0 / 3.0)) * Q30 + 0.5))
    assert gpca.het_weights(np.zeros((0, 4), np.uint32)).shape == (0,)
    with pytest.raises(ValueError):
        gpca.het_weights(np.zeros((3, 3), np.uint32))


def test_sample_het_against_the_restatement():
    rng = np.random.default_rng(2)
    N = 3000
    nobs = rng.integers(1, 200000, N)
    het = (rng.random(N) * nobs).astype(np.int64)
    counts = np.stack([nobs, het, (rng.random(N) * (nobs - het)).astype(np.int64)], 1).astype(np.uint32)
    qsum = (rng.random(N) * 0.5 * nobs * Q30).astype(np.uint64)
    counts[:3] = [[0, 0, 0], [5, 0, 0], [5, 5, 0]]
    qsum[:3] = [0, 0, 0]                                      # no call; no expected heterozygosity (d = 0) twice
    got = gpca.sample_het(counts, qsum)
    want = sample_het_model(counts, qsum)
    assert got.shape == (N, 3) and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(got[:3, 2]).all() and not np.isnan(got[3:]).any()
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0, equal_nan=True)
    # a sample with the expected number of het calls has F = 0; one with none has F = 1
    c = np.array([[1000, 400, 100], [1000, 0, 500]], np.uint32)
    F = gpca.sample_het(c, np.array([400 << 30, 400 << 30], np.uint64))[:, 2]
    assert F[0] == 0.0 and F[1] == 1.0
    assert gpca.sample_het(np.zeros((0, 3), np.uint32), np.zeros(0, np.uint64)).shape == (0, 3)
    with pytest.raises(ValueError):
        gpca.sample_het(c, np.zeros(3, np.uint64))


def test_sample_qc_pass_on_hand_built_tables():
    K = 100
    counts = np.array([[100, 0, 0], [96, 0, 0], [95, 0, 0], [94, 0, 0], [0, 0, 0], [100, 0, 0], [100, 0, 0], [100, 0, 0]], np.uint32)
    nan = float("nan")
    F = np.array([0.0, 0.01, -0.01, 5.0, nan, nan, 0.02, -0.02])
    ok, why = gio.sample_qc_pass(counts, K)                                              # no filter: everyone passes
    assert ok.dtype == np.uint8 and ok.all() and why == [None] * 8
    ok, why = gio.sample_qc_pass(counts, K, mind=0.05)                                   # F_MISS = 0.05 is not above 0.05
    assert ok.tolist() == [1, 1, 1, 0, 0, 1, 1, 1] and why == [None, None, None, "MIND", "MIND", None, None, None]
    ok, why = gio.sample_qc_pass(counts, K, mind=0.0)
    assert ok.tolist() == [1, 0, 0, 0, 0, 1, 1, 1]
    # het alone: NaN fails, and the sample without a call fails HET through its NaN (no MIND rule was asked for); 5.0 stays inside
    # 3 s.d. of a set of six that it inflates itself
    ok, why = gio.sample_qc_pass(counts, K, F, het_sd=3.0)
    assert ok.tolist() == [1, 1, 1, 1, 0, 0, 1, 1] and why[4] == "HET" and why[5] == "HET"
    ok, why = gio.sample_qc_pass(counts, K, F, het_sd=2.0)
    fin = F[[0, 1, 2, 3, 6, 7]]
    m = fin.sum() / 6
    s = np.sqrt(((fin - m) ** 2).sum() / 5)
    assert abs(5.0 - m) > 2.0 * s and ok.tolist() == [1, 1, 1, 0, 0, 0, 1, 1] and why[3] == "HET"
    # both: MIND first; the statistics come from the samples that pass MIND (the 5.0 is gone, so 0.02 is now 2 s.d. out at 1.2)
    ok, why = gio.sample_qc_pass(counts, K, F, mind=0.05, het_sd=1.2)
    fin = F[[0, 1, 2, 6, 7]]
    m = fin.sum() / 5
    s = np.sqrt(((fin - m) ** 2).sum() / 4)
    want = [int(abs(x - m) <= 1.2 * s) for x in F[[0, 1, 2]]] + [0, 0, 0] + [int(abs(x - m) <= 1.2 * s) for x in F[[6, 7]]]
    assert ok.tolist() == want and why[3] == "MIND" and why[4] == "MIND" and why[5] == "HET" and 0 in want[:3] + want[6:]
    # c < 2 or s = 0: only NaN fails
    ok, why = gio.sample_qc_pass(counts[:2], K, np.array([3.0, nan]), het_sd=0.1)
    assert ok.tolist() == [1, 0]
    ok, why = gio.sample_qc_pass(counts[:3], K, np.array([0.5, 0.5, 0.5]), het_sd=0.1)
    assert ok.tolist() == [1, 1, 1]
    with pytest.raises(ValueError):
        gio.sample_qc_pass(counts, K, F[:3], het_sd=3.0)


def test_the_four_writers(tmp_path):
    fids, iids = ["f0", "f0", "f1"], ["a", "b", "c"]
    counts = np.array([[8, 3, 1], [0, 0, 0], [7, 0, 7]], np.uint32)
    pre = str(tmp_path / "sub" / "P")
    assert gio.write_smiss(pre, fids, iids, counts, 8) == pre + ".smiss"
    assert open(pre + ".smiss").read() == ("#FID\tIID\tMISSING_CT\tOBS_CT\tF_MISS\nf0\ta\t0\t8\t0\nf0\tb\t8\t8\t1\nf1\tc\t1\t8\t0.125\n")
    het = np.array([[5.0, 4.5, -0.142857142857], [0.0, 0.0, float("nan")], [7.0, 3.25, 1.0]])
    assert gio.write_het(pre, fids, iids, counts, het) == pre + ".het"
    assert open(pre + ".het").read() == ("#FID\tIID\tO_HOM\tE_HOM\tOBS_CT\tF\nf0\ta\t5\t4.5\t8\t-0.142857\nf0\tb\t0\t0\t0\tNA\nf1\tc\t7\t3.25\t7\t1\n")
    pin, pout = gio.write_sample_qc_ids(pre, fids, iids, np.array([1, 0, 0], np.uint8), [None, "MIND", "HET"])
    assert (pin, pout) == (pre + ".sampleqc.in.id", pre + ".sampleqc.out.id")
    assert open(pin).read() == "#FID\tIID\nf0\ta\n" and open(pout).read() == "#FID\tIID\tREASON\nf0\tb\tMIND\nf1\tc\tHET\n"
    assert gio.sample_count_bands(10, 4) == [(0, 4), (4, 8), (8, 10)] and gio.sample_count_bands(0) == [] and gio.sample_count_bands(5) == [(0, 5)]
    for bad in (lambda: gio.write_smiss(pre, fids, iids, counts[:2], 8), lambda: gio.write_het(pre, fids, iids, counts, het[:2]),
                lambda: gio.write_sample_qc_ids(pre, fids, iids, [1, 1], [None] * 3)):
        with pytest.raises(ValueError):
            bad()


def worked_example(seed=7):
    """400 samples x 5 000 SNPs of one population; returns (G, contaminated, homozygous, sparse)"""
    rng = np.random.default_rng(seed)
    M, N = 5000, 400
    p = rng.uniform(0.1, 0.9, M)[:, None]
    G = (rng.random((M, N)) < p).astype(np.int8) + (rng.random((M, N)) < p).astype(np.int8)
    contaminated, homozygous, sparse = [10, 200], [50, 333], [5, 120, 399]
    for n, other in zip(contaminated, (11, 201)):             # a 50/50 mix of two samples' DNA calls het wherever they differ
        G[:, n] = np.where(G[:, n] != G[:, other], 1, G[:, n])
    for n in homozygous:                                      # 30 % of the het calls come out homozygous
        flip = (G[:, n] == 1) & (rng.random(M) < 0.3)
        G[flip, n] = np.where(rng.random(int(flip.sum())) < 0.5, 0, 2)
    miss = rng.random((M, N)) < 0.005
    for n in sparse:
        miss[:, n] = rng.random(M) < 0.08
    G[miss] = -127
    return G, contaminated, homozygous, sparse


def test_worked_example_flags_exactly_the_seven_bad_samples():
    G, contaminated, homozygous, sparse = worked_example()
    M, N = G.shape
    counts, qc = counts_model(G)
    q = gpca.het_weights(qc)
    obs = G != -127
    qsum = obs.T.astype(np.uint64) @ q.astype(np.uint64)
    het = gpca.sample_het(counts, qsum)
    F = het[:, 2]
    ok, why = gio.sample_qc_pass(counts, M, F, mind=0.05, het_sd=3.0)
    assert sorted(np.flatnonzero(ok == 0).tolist()) == sorted(contaminated + homozygous + sparse)
    assert all(why[n] == "MIND" for n in sparse) and all(why[n] == "HET" for n in contaminated + homozygous)
    assert all(F[n] < -0.3 for n in contaminated) and all(F[n] > 0.2 for n in homozygous)
    good = np.flatnonzero(ok)
    assert abs(F[good].mean()) < 0.01 and F[good].std() < 0.03
