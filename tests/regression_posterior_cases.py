"""The problems shared by tests/test_regression_posterior_restatement.py (CPU) and tests/test_gpu_regression_posterior.py:
a synthetic pair (standard-normal vectors, values in [0.4, 1]), three index styles, both noise models, and per problem
the three reference-form functions of the oracle (np_predict_regression, np_predict_regression_different,
np_posterior_covariance_regression) on its 300 new rows, computed once and shared by every m_new (each a prefix of the 300).
noise + sigma >= 1e-2 throughout (below that the two algebras part by more than 1e-9 of the mean)."""
import functools

import numpy as np

from oracle import flgp_oracle as O

N, KPAIR, PAIR_SEED, MNEW_REF = 3000, 200, 131, 300
MNEW = [1, 15, 16, 17, 63, 64, 65, 300]
STYLES = {            # t, noise, sigma
    "range": (0.5, 0.1, 1e-3),
    "perm_overlap": (2.0, 1e-2, 1e-3),
    "repeat": (4.0, 0.5, 1e-5),
}
# K across the 16-row tile and the row blocks of the fused kernel, m just above K, a few K and many; q = 1, 2, 3 in turn
GRID = [(K, m, 1 + i) for K in (1, 15, 16, 17, 63, 64, 65, 129, 200) for i, m in enumerate((K + 1, 2 * K + 5, 1000))]
# the q mean rows sit in, end at and straddle a 16-row tile of the operand's K + q rows
TILE = [(K, 2 * K + 5, q) for K, q in ((15, 1), (15, 2), (16, 1), (14, 3), (47, 17), (200, 3))]


@functools.lru_cache(maxsize=None)
def host_pair(n=N, K=KPAIR, seed=PAIR_SEED):
    rng = np.random.default_rng(seed)
    values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
    return values, np.asfortranarray(rng.standard_normal((n, K)))


def rows(style, n, m, seed, mnew=MNEW_REF):
    """idx0 and idx1 (mnew rows) of one problem."""
    rng = np.random.default_rng(seed)
    if style == "range":
        start = rng.integers(0, n - mnew - m + 1)
        return np.arange(start, start + m), np.arange(n - mnew, n)
    if style == "perm_overlap":
        perm = rng.permutation(n)
        idx0 = perm[:m]
        shared = min(m, mnew // 3)
        return idx0, rng.permutation(np.r_[idx0[:shared], perm[m:m + mnew - shared]])
    idx0 = rng.integers(0, n, m)
    idx0[m - 1] = idx0[0]
    return idx0, rng.permutation(n)[:mnew]


def references(values, V, Y, idx0, idx1, K, t, nz, sigma):
    """The reference-form results of one problem: nz holds one noise variance per row of idx0; "same" and the variance
    take nz[0] (the drivers' pars = (t, noise[0]), src/Fit.cpp:77)."""
    m = len(idx0)
    pars_d = np.r_[t, nz]
    return dict(
        same=O.np_predict_regression(values, V, Y, idx0, idx1, K, (t, nz[0]), sigma),
        different=O.np_predict_regression_different(values, V, Y, idx0, idx1, K, pars_d, sigma),
        train_same=O.np_predict_regression(values, V, Y, idx0, idx0, K, (t, nz[0]), sigma),
        train_different=O.np_predict_regression_different(values, V, Y, idx0, idx0, K, pars_d, sigma),
        var=O.np_posterior_covariance_regression(values, V, idx0, idx1, K, (t, nz[0]), sigma),
        prior=((V[idx1, :K] ** 2) * np.exp(-t * (1.0 - values[:K]))).sum(1).max(), m=m, c=nz[0] + sigma)


@functools.lru_cache(maxsize=None)
def problem(K, m, q, style):
    values, V = host_pair()
    t, noise, sigma = STYLES[style]
    seed = 7919 * K + 31 * m + q
    idx0, idx1 = rows(style, N, m, seed)
    rng = np.random.default_rng(seed + 1)
    Y = np.asfortranarray(rng.standard_normal((m, q)))
    nz = rng.uniform(0.01, 0.5, m)
    nz[0] = noise
    p = dict(K=K, m=m, q=q, t=t, sigma=sigma, idx0=idx0, idx1=idx1, Y=Y, nz=nz)
    p.update(references(values, V, Y, idx0, idx1, K, t, nz, sigma))
    return p


def atol_mean(ref):
    return 1e-9 * np.abs(ref).max()


def atol_var(p):
    return 1e-9 * np.abs(p["var"]).max() + 2e-15 * p["prior"] * p["m"] / p["c"]
