"""CPU: the algebra of the fitted predictor.  On random host data the restated fold and row kernel
(tests/np_predictor.py), z_i = a_i P with P = Vs diag(sqrt(n) / sigma) [G ; U^T]^T, agree with the weight-space posteriors
(np_regression_posterior.py, np_logit_posterior.py) evaluated on the rows u_i = a_i Vs diag(sqrt(n) / sigma) that the
extension would store -- to the tolerance forms of tests/regression_posterior_cases.py and np_logit_posterior.tolerances."""
import numpy as np
import pytest
import scipy.linalg as sl

import np_logit_posterior as nlp
import np_predictor as npp
import np_regression_posterior as nrp
import regression_posterior_cases as rc

S, N_FIT, N_NEW = 30, 700, 41


def _setting(K, r, seed):
    """a pair of m + n_new rows made as the extension makes them: anchor eigenvectors, eigenvalues (one of them 0 for
    K > 1: a zero column of U-recovery), sparse rows with ascending indices, u = a Vs diag(sqrt(n) / sigma)"""
    rng = np.random.default_rng(seed)
    m = 2 * K + 5
    n = m + N_NEW
    Vs = rng.standard_normal((S, K))
    eig = rng.uniform(0.2, 1.0, K)
    if K > 1:
        eig[K - 1] = 0.0
    values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
    idx = np.sort(np.stack([rng.permutation(S)[:r] for _ in range(n)]), axis=1)
    val = rng.uniform(0.0, 1.0, (n, r)) / np.sqrt(N_FIT)
    Bq = npp.anchor_side(Vs, eig, N_FIT, K)
    u = np.zeros((n, K))
    for a in range(r):
        u += val[:, a:a + 1] * Bq[idx[:, a]]
    return dict(K=K, m=m, n=n, Vs=Vs, eig=eig, values=values, idx=idx, val=val, u=u, idx0=np.arange(m), idx1=np.arange(m, n))


def _regression_operand(c, Y, t, noise, sigma):
    """G = sqrt(c) L_Q^-1 L^1/2 and U = L^1/2 beta of the header's formulas ("same"; noise an array: "different")"""
    K, V1 = c["K"], c["u"][c["idx0"]]
    ls = np.sqrt(nrp.lam_of(c["values"], K, t))
    nz = np.asarray(noise, dtype=np.float64)
    cc = float(nz.reshape(-1)[0]) + sigma
    Qs = (ls[:, None] * (V1.T @ V1)) * ls[None, :] + cc * np.eye(K)
    if nz.ndim == 0:
        Qd, rhs = Qs, ls[:, None] * (V1.T @ Y)
    else:
        zinv = 1.0 / (nz + sigma)
        Qd = (ls[:, None] * (V1.T @ (zinv[:, None] * V1))) * ls[None, :] + np.eye(K)
        rhs = ls[:, None] * (V1.T @ (zinv[:, None] * Y))
    beta = sl.cho_solve(sl.cho_factor(Qd, lower=True), rhs)
    G = sl.solve_triangular(np.linalg.cholesky(Qs), np.eye(K), lower=True) * (np.sqrt(cc) * ls)[None, :]
    return G, ls[:, None] * beta, cc


@pytest.mark.parametrize("noisepar", ["same", "different"])
@pytest.mark.parametrize("r", [1, 5])
@pytest.mark.parametrize("q", [1, 3])
@pytest.mark.parametrize("K", [1, 20, 65])
def test_regression_rows_from_the_folded_operand(K, q, r, noisepar):
    c = _setting(K, r, seed=100 * K + 10 * q + r)
    rng = np.random.default_rng(K + q)
    t, sigma = 2.0, 1e-3
    Y = rng.standard_normal((c["m"], q))
    nz = rng.uniform(0.01, 0.5, c["m"])
    noise = nz[0] if noisepar == "same" else nz
    G, U, cc = _regression_operand(c, Y, t, noise, sigma)
    P = npp.fold(c["Vs"], c["eig"], N_FIT, G, U)
    assert P.shape == (S, K + q)
    mean, var = npp.rows(c["idx"][c["idx1"]], c["val"][c["idx1"]], P, 1, K, q, [cc])
    ref_mean = nrp.weight_space_mean(c["values"], c["u"], Y, c["idx0"], c["idx1"], K, t, noise, sigma)
    ref_var = nrp.weight_space_variance(c["values"], c["u"], c["idx0"], c["idx1"], K, t, nz[0], sigma)
    prior = ((c["u"][c["idx1"]] ** 2) * nrp.lam_of(c["values"], K, t)).sum(1).max()
    p = dict(var=ref_var, prior=prior, m=c["m"], c=cc)
    assert np.abs(mean - ref_mean).max() <= rc.atol_mean(ref_mean)
    assert np.abs(var[:, 0] - ref_var).max() <= rc.atol_var(p)
    assert (var >= cc).all()


@pytest.mark.parametrize("sig", [(0.0, 1e-3), (0.05, 0.0)])
def test_logit_rows_from_the_folded_operand(sig):
    K, r = 20, 5
    c = _setting(K, r, seed=77)
    Y = np.random.default_rng(3).integers(0, 2, c["m"]).astype(np.float64)
    t = 1.5
    beta, LQ, _, _ = nlp.weight_space_mode(c["values"], c["u"], K, t, c["idx0"], Y, sig[0])
    ls = np.sqrt(nlp.lam_of(c["values"], K, t))
    G = sl.solve_triangular(LQ, np.eye(K), lower=True) * ls[None, :]
    P = npp.fold(c["Vs"], c["eig"], N_FIT, G, ls * beta)
    mean, var = npp.rows(c["idx"][c["idx1"]], c["val"][c["idx1"]], P, 1, K, 1, [sig[1]])
    ref_mean, ref_var = nlp.predict(c["values"], c["u"], K, t, c["idx1"], beta, LQ, sig[1])
    C22 = ((c["u"][c["idx1"]] ** 2) * nlp.lam_of(c["values"], K, t)).sum(1) + sig[1]
    am, av = nlp.tolerances(ref_mean, ref_var, C22, c["m"])
    assert np.abs(mean[:, 0] - ref_mean).max() <= am
    assert np.abs(var[:, 0] - ref_var).max() <= av
    assert (var >= sig[1]).all()


def test_the_sum_of_squares_order_is_the_stated_one():
    """K = 130 on one row, written out lane by lane: S_l over k = l, l + 64, l + 128, then the six butterfly steps."""
    rng = np.random.default_rng(9)
    K, q = 130, 2
    P = rng.standard_normal((4, K + q))
    idx = np.array([[1, 3]]); val = rng.standard_normal((1, 2))
    mean, var = npp.rows(idx, val, P, 1, K, q, [0.25])
    z = (0.0 + val[0, 0] * P[1]) + val[0, 1] * P[3]
    np.testing.assert_array_equal(mean[0], z[K:])
    S = [0.0] * 64
    for k in range(K):
        S[k % 64] = S[k % 64] + z[k] * z[k]
    for o in (32, 16, 8, 4, 2, 1):
        S = [S[l] + S[l ^ o] for l in range(64)]
    assert var[0, 0] == 0.25 + S[0]
    assert len(set(S)) == 1                                    # every lane ends with the same bits
