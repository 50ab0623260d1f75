"""The admixture simulation shared by tests/test_fstat_host.py and tests/test_cpp_fstats.py: the tree ((A, B), (C, D)) with X = A / 2 + C / 2.

Per SNP the root frequency is uniform on (0.1, 0.9); the two inner nodes drift from it with F = 0.05, A and B from the first and C and D
from the second with F = 0.02 (a child's frequency is Beta(p (1 - F) / F, (1 - p) (1 - F) / F)); X has frequency (p_A + p_C) / 2.  30
diploid samples per population, a fraction `miss` of the calls missing.  Expected: f3(X; A, C) = -f2(A, C) / 4 < 0, f4(A, B; C, D) = 0
and f4(A, C; B, D) = the drift of the inner branch > 0."""
import numpy as np

POPS = ["A", "B", "C", "D", "X"]
F_INNER, F_LEAF = 0.05, 0.02


def drift(rng, p, F):
    return rng.beta(p * (1 - F) / F, (1 - p) * (1 - F) / F)


def simulate(seed, M=20000, n=30, miss=0.02):
    """(G int8 [M][5 n] with -127 for a missing call, pop int32 [5 n] = the index into POPS)"""
    rng = np.random.default_rng(seed)
    root = rng.uniform(0.1, 0.9, M)
    ab, cd = drift(rng, root, F_INNER), drift(rng, root, F_INNER)
    f = {"A": drift(rng, ab, F_LEAF), "B": drift(rng, ab, F_LEAF), "C": drift(rng, cd, F_LEAF), "D": drift(rng, cd, F_LEAF)}
    f["X"] = 0.5 * f["A"] + 0.5 * f["C"]
    pop = np.repeat(np.arange(len(POPS)), n).astype(np.int32)
    G = np.zeros((M, len(pop)), np.int8)
    for k, name in enumerate(POPS):
        p = f[name][:, None]
        G[:, pop == k] = (rng.random((M, n)) < p).astype(np.int8) + (rng.random((M, n)) < p).astype(np.int8)
    G[rng.random(G.shape) < miss] = -127
    return G, pop
