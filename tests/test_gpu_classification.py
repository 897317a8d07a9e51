"""GPU: the Laplace-approximation classification consumers against a numpy restatement of GPML Alg. 3.1 /
3.2 as the reference writes them -- marginal_log_likelihood_logit_la_cpp (src/train.cpp:716-760) and
posterior_distribution_classification (src/Utils.cpp:252-299), with C21 formed densely here."""
import numpy as np
import pytest
import scipy.linalg as sl

from flgp_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does (as the parity suite's
    fixtures do), or torch finds no GPU for the rest of the process."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()


# ---- numpy restatement ------------------------------------------------------------------------------------------------
def np_newton(C, Y, N, tol=1e-5, max_iter=100, binomial=True):
    """Alg. 3.1 from f = 0; returns (f, a, L of the last iteration, iterations)."""
    m = Y.size
    f = np.zeros(m)
    it = 0
    for it in range(1, max_iter + 1):
        pi = 1.0 / (1.0 + np.exp(-f))
        W = N * pi * (1 - pi) if binomial else pi * (1 - pi)
        sW = np.sqrt(W)
        B = sW[:, None] * C * sW[None, :] + np.eye(m)
        L = np.linalg.cholesky(B)
        b = W * f + Y * (1 - pi) + (N - Y) * (-pi) if binomial else W * f + (Y - pi)
        a = b - sW * sl.cho_solve((L, True), sW * (C @ b))
        f_new = C @ a
        done = np.abs(f - f_new).sum() < tol
        f = f_new
        if done:
            break
    return f, a, L, it


def np_amll(C, Y, N, tol=1e-5, max_iter=100):
    f, a, L, it = np_newton(C, Y, N, tol, max_iter)
    pi = 1.0 / (1.0 + np.exp(-f))
    amll = -0.5 * (a * f).sum() + (Y * np.log(pi)).sum() + ((N - Y) * np.log(1 - pi)).sum()
    amll -= np.log(np.diag(L) + 1e-9).sum()
    return amll, it


def np_posterior(C11, C21, C22, Y, tol=1e-5, max_iter=100):
    f, _, _, _ = np_newton(C11, Y, np.ones(Y.size), tol, max_iter, binomial=False)
    pi = 1.0 / (1.0 + np.exp(-f))
    sW = np.sqrt(pi * (1 - pi))
    B = sW[:, None] * C11 * sW[None, :] + np.eye(Y.size)
    beta = sW[:, None] * sl.cho_solve((np.linalg.cholesky(B), True), np.eye(Y.size)) * sW[None, :]
    mean = C21 @ (Y - pi)
    cov = C22 - ((C21 @ beta) * C21).sum(1)
    return mean, cov


def hk(values, V, K, t, i0, i1):
    lam = np.exp(-t * (1.0 - values[:K]))
    return (V[i0, :K] * lam) @ V[i1, :K].T


def spd(m, rng, amp=4.0):
    """An RBF kernel matrix on random points plus a small ridge (a GP covariance, exactly symmetric)."""
    x = rng.uniform(-3, 3, size=(m, 2))
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    C = amp * np.exp(-0.5 * d2) + 1e-3 * np.eye(m)
    return np.asfortranarray(0.5 * (C + C.T)), x


def labels(x, rng, N):
    p = 1.0 / (1.0 + np.exp(-2.0 * np.sin(x[:, 0]) * np.cos(x[:, 1])))
    return rng.binomial(N.astype(int), p).astype(np.float64)


def synthetic_pair(n, K, seed):
    rng = np.random.default_rng(seed)
    values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
    V = np.asfortranarray(rng.standard_normal((n, K)))
    return api.EigenPair(values, V), api.ResidentEigenPair.from_host(api.EigenPair(values, V))


# ---- host-C entry -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 7, 63, 64, 65, 300, 1000, 2500])
@pytest.mark.parametrize("binomial", [False, True])
def test_logit_la_host_matrix(m, binomial):
    rng = np.random.default_rng(1000 * m + binomial)
    C, x = spd(m, rng)
    N = rng.integers(1, 6, m).astype(np.float64) if binomial else np.ones(m)
    Y = labels(x, rng, N)
    ref, it_ref = np_amll(C, Y, N)
    got, it = api.marginal_log_likelihood_logit_la_cpp(C, Y, N, return_iters=True)
    assert it == it_ref
    assert abs(got - ref) <= 1e-10 * abs(ref), (got, ref)


def test_logit_la_max_iter_is_not_an_error():
    rng = np.random.default_rng(5)
    C, x = spd(200, rng)
    Y = labels(x, rng, np.ones(200))
    got, it = api.marginal_log_likelihood_logit_la_cpp(C, Y, np.ones(200), max_iter=2, return_iters=True)
    ref, it_ref = np_amll(C, Y, np.ones(200), max_iter=2)
    assert it == it_ref == 2
    assert abs(got - ref) <= 1e-10 * abs(ref)


# ---- the blocked factorisation on its own -----------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 129, 700])
def test_blocked_cholesky_and_solves(m):
    import torch
    from flgp_amd import _lib
    rng = np.random.default_rng(m)
    C, _ = spd(m, rng)
    C += np.eye(m)
    L_ref = np.linalg.cholesky(C)
    dA = torch.tensor(C.T.copy(), device="cuda")            # row-major of C^T = column-major of C
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().flgp_dev_cholesky(None, dA.data_ptr(), m, 0, flag.data_ptr()))
    dB = torch.tensor(rng.standard_normal((3, m)), device="cuda")   # 3 right-hand sides, column-major
    B = dB.cpu().numpy().T.copy()
    _lib.check(_lib.lib().flgp_dev_chol_solve(None, dA.data_ptr(), m, dB.data_ptr(), 3, 3, flag.data_ptr()))
    torch.cuda.synchronize()
    assert flag.item() == 0
    L = np.tril(dA.cpu().numpy().T)
    np.testing.assert_allclose(L, L_ref, rtol=0, atol=1e-12 * np.abs(L_ref).max())
    X = sl.cho_solve((L_ref, True), B)
    np.testing.assert_allclose(dB.cpu().numpy().T, X, rtol=0, atol=1e-10 * np.abs(X).max())
    # the one-workgroup factorisation of the regression entries gives the same factor
    dS = torch.tensor(C.T.copy(), device="cuda")
    _lib.check(_lib.lib().flgp_dev_cholesky(None, dS.data_ptr(), m, 1, flag.data_ptr()))
    torch.cuda.synchronize()
    np.testing.assert_allclose(np.tril(dS.cpu().numpy().T), L_ref, rtol=0, atol=1e-12 * np.abs(L_ref).max())


# ---- resident entry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,m,perm", [(50, 300, False), (50, 300, True), (200, 150, False), (200, 150, True)])
def test_resident_marginal_likelihood_equals_host_entry(K, m, perm):
    n = 3000
    ep, rp = synthetic_pair(n, 240, seed=K + m)
    rng = np.random.default_rng(K * m)
    idx = rng.permutation(n)[:m] if perm else np.arange(100, 100 + m)
    Y = (rng.uniform(size=m) < 0.4).astype(np.float64)
    N = np.ones(m)
    for t, sigma in [(3.0, 1e-3), (0.5, 0.1)]:
        C = rp.HK_from_spectrum_cpp(K, t, idx, idx) + sigma * np.eye(m)
        host, it_h = api.marginal_log_likelihood_logit_la_cpp(C, Y, N, return_iters=True)
        got, it = rp.marginal_log_likelihood_logit_la(K, t, idx, Y, N, sigma=sigma, return_iters=True)
        assert it == it_h
        assert abs(got - host) <= 1e-12 * abs(host), (got, host)
        ref, it_ref = np_amll(hk(ep.values, ep.vectors, K, t, idx, idx) + sigma * np.eye(m), Y, N)
        assert it == it_ref and abs(got - ref) <= 1e-10 * abs(ref)
    rp.free()


# ---- posterior --------------------------------------------------------------------------------------------------------
def check_posterior(post, ep, K, t, idx0, idx1, Y, sigma11, sigma22):
    C11 = hk(ep.values, ep.vectors, K, t, idx0, idx0) + sigma11 * np.eye(idx0.size)
    C21 = hk(ep.values, ep.vectors, K, t, idx1, idx0)
    lam = np.exp(-t * (1.0 - ep.values[:K]))
    C22 = ((ep.vectors[idx1, :K] ** 2) * lam).sum(1) + sigma22
    mean, cov = np_posterior(C11, C21, C22, Y)
    np.testing.assert_allclose(post["mean"], mean, rtol=0, atol=1e-9 * np.abs(mean).max())
    # var = C22 - (a term of size C22 * m * max W, W <= 1/4): two correct fp64 evaluations differ by that times a few eps
    allowance = 2e-15 * C22.max() * idx0.size * 0.25
    np.testing.assert_allclose(post["cov"], cov, rtol=0, atol=1e-9 * np.abs(cov).max() + allowance)
    assert (post["cov"] > 0).all()


@pytest.mark.parametrize("sigmas", [(1e-3, 1e-3), (0.0, 1e-3)])
def test_posterior_classification_against_dense(sigmas):
    n, K, m = 6000, 80, 400
    ep, rp = synthetic_pair(n, 100, seed=3)
    rng = np.random.default_rng(4)
    for idx0, idx1 in [(np.arange(m), np.arange(m, m + 2000)), (rng.permutation(n)[:m], rng.permutation(n)[:2000])]:
        Y = (rng.uniform(size=m) < 0.5).astype(np.float64)
        t = 2.0
        post = rp.posterior_distribution_classification(idx0, idx1, K, t, Y, *sigmas)
        check_posterior(post, ep, K, t, idx0, idx1, Y, *sigmas)
        again = rp.posterior_distribution_classification(idx0, idx1, K, t, Y, *sigmas)
        assert np.array_equal(post["mean"], again["mean"]) and np.array_equal(post["cov"], again["cov"])
    rp.free()


def test_posterior_classification_baseline_shape():
    """BASELINE configs[2] shape: n = 1e6, K = 200, m = 1000, m_new = 999 000; 2000 new rows checked densely."""
    n, K, m = 1_000_000, 200, 1000
    ep, rp = synthetic_pair(n, K, seed=11)
    rng = np.random.default_rng(12)
    idx0 = np.arange(m); idx1 = np.arange(m, n)
    Y = (rng.uniform(size=m) < 0.3).astype(np.float64)
    t, sigma = 4.0, 1e-3
    post = rp.posterior_distribution_classification(idx0, idx1, K, t, Y, sigma, sigma)
    assert post["mean"].shape == (n - m,) and (post["cov"] > 0).all()
    sample = np.sort(rng.choice(n - m, 2000, replace=False))
    check_posterior({"mean": post["mean"][sample], "cov": post["cov"][sample]}, ep, K, t, idx0, idx1[sample], Y, sigma, sigma)
    rp.free()


def test_posterior_multiclassification_against_numpy_loop():
    n, K, m = 4000, 60, 300
    ep, rp = synthetic_pair(n, 60, seed=21)
    rng = np.random.default_rng(22)
    idx0 = rng.permutation(n)[:m]; idx1 = np.arange(n - 1500, n)
    Y = rng.integers(0, 3, m).astype(np.float64)
    ts = [1.0, 2.5, 4.0]
    sigma = 1e-3
    post = rp.posterior_distribution_multiclassification(idx0, idx1, K, ts, Y, sigma)
    assert post["mean"].shape == (idx1.size, 3)
    aug = api.multi_train_split(Y)
    for j in range(3):
        check_posterior({"mean": post["mean"][:, j], "cov": post["cov"][:, j]}, ep, K, ts[j], idx0, idx1, aug[:, j], 0.0, sigma)
    rp.free()


# ---- block edges of the resident entries -----------------------------------------------------------------------------
# m = 1 and 65 (one and two panels of chol_blocked / chol_trsv), m_new = 1, and K = 64, 65, 129 right-hand sides of
# chol_trsv mode 1 in the posterior (L_B^-1 sqrt(W) V1 L: one workgroup per column of V1)
@pytest.mark.parametrize("m,K,mnew", [(1, 50, 1), (1, 65, 300), (65, 50, 1), (65, 64, 300), (200, 65, 129), (300, 129, 1)])
def test_resident_block_edges(m, K, mnew):
    n = 3000
    ep, rp = synthetic_pair(n, 130, seed=m + K)
    rng = np.random.default_rng(m * K + mnew)
    idx0 = rng.permutation(n)[:m]; idx1 = rng.permutation(n)[:mnew]
    Y = (rng.uniform(size=m) < 0.4).astype(np.float64)
    t, sigma = 2.0, 1e-3
    got, it = rp.marginal_log_likelihood_logit_la(K, t, idx0, Y, sigma=sigma, return_iters=True)
    ref, it_ref = np_amll(hk(ep.values, ep.vectors, K, t, idx0, idx0) + sigma * np.eye(m), Y, np.ones(m))
    assert it == it_ref and abs(got - ref) <= 1e-10 * abs(ref), (got, ref)
    post = rp.posterior_distribution_classification(idx0, idx1, K, t, Y, sigma, sigma)
    assert post["mean"].shape == (mnew,) and post["cov"].shape == (mnew,)
    check_posterior(post, ep, K, t, idx0, idx1, Y, sigma, sigma)
    rp.free()


def test_posterior_multiclassification_k65():
    n, K, m = 3000, 65, 150
    ep, rp = synthetic_pair(n, K, seed=23)
    rng = np.random.default_rng(24)
    idx0 = rng.permutation(n)[:m]; idx1 = np.arange(n - 129, n)
    Y = rng.integers(0, 3, m).astype(np.float64)
    ts = [1.0, 2.5, 4.0]
    sigma = 1e-3
    post = rp.posterior_distribution_multiclassification(idx0, idx1, K, ts, Y, sigma)
    assert post["mean"].shape == (idx1.size, 3)
    aug = api.multi_train_split(Y)
    for j in range(3):
        check_posterior({"mean": post["mean"][:, j], "cov": post["cov"][:, j]}, ep, K, ts[j], idx0, idx1, aug[:, j], 0.0, sigma)
    rp.free()


# ---- errors, determinism ----------------------------------------------------------------------------------------------
def test_errors():
    n = 2000
    ep, rp = synthetic_pair(n, 40, seed=31)
    idx = np.arange(100); Y = np.zeros(100); Y[::3] = 1
    with pytest.raises(api.FlgpError) as e:                        # C = HK - 50 I: indefinite
        rp.marginal_log_likelihood_logit_la(40, 1.0, idx, Y, sigma=-50.0)
    assert e.value.code == -5 and "pivot" in e.value.message
    with pytest.raises(api.FlgpError) as e:
        rp.posterior_distribution_classification(idx, np.arange(5), 40, 1.0, Y, -50.0, 0.0)
    assert e.value.code == -5 and "pivot" in e.value.message
    with pytest.raises(api.FlgpError) as e:                        # Y outside [0, N]
        rp.marginal_log_likelihood_logit_la(40, 1.0, idx, Y + 1.5)
    assert e.value.code == -1 and "outside" in e.value.message
    with pytest.raises(api.FlgpError) as e:                        # row out of range
        rp.marginal_log_likelihood_logit_la(40, 1.0, np.append(idx[:-1], n), Y)
    assert e.value.code == -1 and "out of range" in e.value.message
    with pytest.raises(api.FlgpError) as e:
        rp.posterior_distribution_classification(idx, np.array([0, n]), 40, 1.0, Y, 1e-3, 1e-3)
    assert e.value.code == -1 and "out of range" in e.value.message
    with pytest.raises(api.FlgpError) as e:                        # K beyond the stored pairs
        rp.marginal_log_likelihood_logit_la(41, 1.0, idx, Y)
    assert e.value.code == -1
    with pytest.raises(api.FlgpError) as e:
        rp.posterior_distribution_classification(idx, np.arange(5), 41, 1.0, Y, 1e-3, 1e-3)
    assert e.value.code == -1
    # the library still works after the refusals
    assert np.isfinite(rp.marginal_log_likelihood_logit_la(40, 1.0, idx, Y))
    rp.free()


def test_determinism():
    rng = np.random.default_rng(41)
    C, x = spd(1000, rng)
    N = rng.integers(1, 4, 1000).astype(np.float64)
    Y = labels(x, rng, N)
    a = api.marginal_log_likelihood_logit_la_cpp(C, Y, N)
    b = api.marginal_log_likelihood_logit_la_cpp(C, Y, N)
    assert a == b
