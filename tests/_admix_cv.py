"""Helpers of the admixture cross-validation tests (include/gpca.h section a22): numpy restatements of the fold rule, of a21's step, fit
and init in f64, and the derived log-likelihood bar.  Restated here, not imported from another test module."""
import numpy as np

U = 2.0 ** -24
EPS = np.float32(1e-5)
HI = np.float32(1.0) - np.float32(1e-5)
C_LOG = 3.0               # the device logf's measured error bound in units of u |log p| (tests/test_gpu_admix.py measures and holds it)
MISSING = -127
STREAM_CV = 0x41444D43


def philox(c0, c1, c2, c3, k0, k1):
    """philox4x32-10 on uint64 arrays holding 32-bit words: [..., 4]"""
    M32 = np.uint64(0xffffffff)
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack([c0, c1, c2, c3], -1)


def folds_np(seed, v, rows, N, row0=0):
    """a22's fold of the kept rows row0 .. row0 + rows - 1 and the samples 0 .. N - 1: uint8 [rows][N].  w = word i & 3 of
    philox(counter = (j, i >> 2, 0, stream), key = the seed's words); fold = (w v) >> 32"""
    q0, q1 = row0 >> 2, (row0 + max(rows, 1) - 1) >> 2
    quad = np.arange(q0, q1 + 1, dtype=np.uint64)[:, None]
    j = np.arange(N, dtype=np.uint64)[None, :]
    w = philox(j, quad, 0, STREAM_CV, seed & 0xffffffff, (seed >> 32) & 0xffffffff)          # [quads][N][4]
    f = ((w * np.uint64(v)) >> np.uint64(32)).astype(np.uint8)
    f = f.transpose(0, 2, 1).reshape(-1, N)                                                # row 4 quad + word
    return f[row0 - 4 * q0:row0 - 4 * q0 + rows]


def hold(Gk, fold, c):
    """the kept rows with the observed calls of fold c overwritten by the missing code"""
    out = Gk.copy()
    out[(fold == c) & (Gk != MISSING)] = MISSING
    return out


def ll_bar(K, n_obs, ll_ref):
    """|l - l_ref| of n_obs observed calls: p carries (2 K + 4) u, two terms per call, plus logf's own error"""
    return 2.0 * (2 * K + 4) * U * 2.0 * n_obs + C_LOG * U * abs(ll_ref)


def loglik64(Gk, Q, F, where=None):
    """the f64 log-likelihood of the observed calls of Gk (those under `where`, if given)"""
    Q, F = np.asarray(Q, np.float64), np.asarray(F, np.float64)
    obs = Gk != MISSING
    if where is not None:
        obs = obs & where
    g = np.where(obs, Gk, 0).astype(np.float64)
    p1, p0 = F @ Q.T, (1.0 - F) @ Q.T
    w1, w0 = g * obs, (2.0 - g) * obs
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(w1 > 0, w1 * np.log(p1), 0.0).sum() + np.where(w0 > 0, w0 * np.log(p0), 0.0).sum())


def model_step(Gk, Q, F, mode=None):
    """a21's step in f64 on the kept rows Gk: (Q', F', loglik)"""
    Q, F = np.asarray(Q, np.float64), np.asarray(F, np.float64)
    N = Q.shape[0]
    mode = np.zeros(N, np.uint8) if mode is None else np.asarray(mode)
    obs = Gk != MISSING
    g = np.where(obs, Gk, 0).astype(np.float64)
    p1, p0 = F @ Q.T, (1.0 - F) @ Q.T
    w1, w0 = g * obs, (2.0 - g) * obs
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b = np.where(w1 > 0, w1 / p1, 0.0), np.where(w0 > 0, w0 / p0, 0.0)
        ll = float(np.where(w1 > 0, w1 * np.log(p1), 0.0).sum() + np.where(w0 > 0, w0 * np.log(p0), 0.0).sum())
        c = mode != 2
        AQ, BQ = a[:, c] @ Q[c], b[:, c] @ Q[c]
        num = F * AQ
        den = num + (1.0 - F) * BQ
        Fn = np.where(den > 0, np.clip(num / den, float(EPS), float(HI)), F)
        t = Q * (a.T @ F + b.T @ (1.0 - F))
        tot = t.sum(1, keepdims=True)
        x = np.maximum(t / tot, float(EPS))
        Qn = np.where((mode[:, None] == 1) | ~(tot > 0), Q, x / x.sum(1, keepdims=True))
    return Qn, Fn, ll


def model_fit(Gk, Q, F, tol, max_iter=5000):
    """a21's accelerated fit in f64 from (Q, F), every sample free: (Q, F, steps)"""
    t0 = (np.asarray(Q, np.float64), np.asarray(F, np.float64))
    steps, prev = 0, None
    while steps < max_iter:
        q1, f1, l0 = model_step(Gk, *t0); steps += 1
        if prev is not None and l0 - prev < tol * abs(l0):
            return q1, f1, steps
        prev = l0
        if steps >= max_iter:
            t0 = (q1, f1); continue
        q2, f2, l1 = model_step(Gk, q1, f1); steps += 1
        rq, rf = q1 - t0[0], f1 - t0[1]
        vq, vf = q2 - q1 - rq, f2 - f1 - rf
        nr, nv = np.sqrt((rq ** 2).sum() + (rf ** 2).sum()), np.sqrt((vq ** 2).sum() + (vf ** 2).sum())
        if not nv > 0 or steps >= max_iter:
            t0 = (q2, f2); continue
        al = min(-nr / nv, -1.0)
        fx = np.clip(t0[1] - 2 * al * rf + al * al * vf, float(EPS), float(HI))
        qx = np.maximum(t0[0] - 2 * al * rq + al * al * vq, float(EPS))
        qx = qx / qx.sum(1, keepdims=True)
        q3, f3, lx = model_step(Gk, qx, fx); steps += 1
        t0 = (q3, f3) if lx >= l1 else (q2, f2)
    return t0[0], t0[1], steps


def deviance(held_loglik, n_het_held):
    """a22: the summed squared binomial deviance residuals of a fold"""
    return -2.0 * held_loglik - 4.0 * np.log(2.0) * n_het_held


def model_cv(Gk, Q0, F0, fold, v, tol):
    """a22's cross-validation error of the f64 model from (Q0, F0) with the given folds: (cv_error, per-fold deviance / n_held)"""
    dev, held, per = 0.0, 0, []
    for c in range(v):
        q, f, _ = model_fit(hold(Gk, fold, c), Q0, F0, tol)
        m = (fold == c) & (Gk != MISSING)
        d = deviance(loglik64(Gk, q, f, m), int((Gk[m] == 1).sum()))
        dev += d; held += int(m.sum()); per.append(d / max(int(m.sum()), 1))
    return dev / held, per


def uniforms(stream, n, K, seed):
    """u [n][K] of a21: ((w >> 9) + 0.5) 2^-23, w = word k & 3 of philox(index, k >> 2, stream; seed)"""
    idx = np.arange(n, dtype=np.uint64)
    out = np.zeros((n, K), np.float32)
    for blk in range((K + 3) // 4):
        w = philox(idx & np.uint64(0xffffffff), idx >> np.uint64(32), blk, stream, seed & 0xffffffff, (seed >> 32) & 0xffffffff)
        for k in range(4 * blk, min(4 * blk + 4, K)):
            out[:, k] = ((w[:, k & 3] >> np.uint64(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    return out


def model_init(Gk, K, seed):
    """a21's init of the kept rows Gk (every sample's calls counted)"""
    N = Gk.shape[1]
    x = np.float32(0.1) + np.float32(0.9) * uniforms(0x41444D51, N, K, seed)
    s = np.zeros(N, np.float32)
    for k in range(K):
        s = s + x[:, k]
    Q = x / s[:, None]
    nv, nhet, nh2 = (Gk != MISSING).sum(1).astype(np.float64), (Gk == 1).sum(1).astype(np.float64), (Gk == 2).sum(1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        freq = np.where(nv > 0, (nhet + 2.0 * nh2) / (2.0 * nv), 0.5).astype(np.float32)
    f = freq[:, None] * (np.float32(0.5) + uniforms(0x41444D46, Gk.shape[0], K, seed))
    return Q.astype(np.float32), np.clip(f, EPS, HI).astype(np.float32)


def simulate(M=600, N=96, K=3, fst=0.1, seed=2024):
    """Balding-Nichols frequencies (Fst 0.1), Q ~ Dirichlet(0.3) with 10 pure samples per ancestry, 2 % missing"""
    rng = np.random.default_rng(seed)
    pa = rng.uniform(0.05, 0.95, M)
    Ft = np.clip(rng.beta(pa[:, None] * (1 - fst) / fst, (1 - pa[:, None]) * (1 - fst) / fst, (M, K)), 1e-3, 1 - 1e-3)
    Qt = rng.dirichlet(np.full(K, 0.3), N)
    for k in range(K):
        Qt[10 * k:10 * k + 10] = np.eye(K)[k]
    G = rng.binomial(2, Ft @ Qt.T).astype(np.int8)
    G[rng.random((M, N)) < 0.02] = MISSING
    return G
