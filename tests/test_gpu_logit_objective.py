"""GPU: the logit training objective on the resident pair (flgp_eigenpair_logit_objective) -- the value
train_lae_logit_gp_cpp's COBYLA minimises (src/train.cpp:14-34).  m <= K: the dense loop of the existing entry, bit for
bit; m > K: the low-rank Newton loop against numpy restatements of both the dense (reference) loop and the low-rank one."""
import ctypes

import numpy as np
import pytest
import scipy.linalg as sl

from flgp_amd import _lib, api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does (as the parity suite's
    fixtures do), or torch finds no GPU for the rest of the process."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()


# ---- numpy restatements -----------------------------------------------------------------------------------------------
def np_newton(C, Y, N, tol=1e-5, max_iter=100, binomial=True):
    """Alg. 3.1 from f = 0 (src/train.cpp:716-760); returns (f, a, L of the last iteration, iterations)."""
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
    """amll as the reference writes it; also returns the last iteration's factor of B."""
    f, a, L, it = np_newton(C, Y, N, tol, max_iter)
    pi = 1.0 / (1.0 + np.exp(-f))
    amll = -0.5 * (a * f).sum() + (Y * np.log(pi)).sum() + ((N - Y) * np.log(1 - pi)).sum()
    amll -= np.log(np.diag(L) + 1e-9).sum()
    return amll, it, L


def np_lowrank(V1, lam, sigma, Y, N, tol=1e-5, max_iter=100):
    """The m > K route as include/flgp_hip.h states it: C = V1 diag(lam) V1^T + sigma I never formed, B solved through
    Q = I + X^T X with X = diag(sqrt(W / D)) V1 diag(sqrt(lam)), D = 1 + sigma W; log det B = sum log D + log det Q."""
    m = Y.size
    ls = np.sqrt(lam)
    cmul = lambda x: V1 @ (lam * (V1.T @ x)) + sigma * x   # noqa: E731
    f = np.zeros(m)
    it = 0
    for it in range(1, max_iter + 1):
        pi = 1.0 / (1.0 + np.exp(-f))
        W = N * pi * (1 - pi)
        sW = np.sqrt(W)
        b = W * f + Y * (1 - pi) + (N - Y) * (-pi)
        D = 1.0 + sigma * W
        dh = 1.0 / np.sqrt(D)
        xs = sW * dh
        X = xs[:, None] * V1 * ls[None, :]
        LQ = np.linalg.cholesky(np.eye(V1.shape[1]) + X.T @ X)
        g = xs * cmul(b)
        Xv = X @ sl.cho_solve((LQ, True), X.T @ g)
        a = b - sW * (dh * (g - Xv))
        f_new = cmul(a)
        done = np.abs(f - f_new).sum() < tol
        f = f_new
        if done:
            break
    pi = 1.0 / (1.0 + np.exp(-f))
    amll = -0.5 * (a * f).sum() + (Y * np.log(pi)).sum() + ((N - Y) * np.log(1 - pi)).sum()
    amll -= 0.5 * np.log(D).sum() + np.log(np.diag(LQ)).sum()
    return amll, it


def prior_term(t, prior=(1e-2, 10.0, 2.0)):
    p, q, tau = prior
    return p * np.log(t + 1e-9) + (t / tau) ** (-q)


def hk(values, V, K, t, i0, i1):
    lam = np.exp(-t * (1.0 - values[:K]))
    return (V[i0, :K] * lam) @ V[i1, :K].T


def synthetic_pair(n, K, seed):
    rng = np.random.default_rng(seed)
    values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
    V = np.asfortranarray(rng.standard_normal((n, K)))
    return api.EigenPair(values, V), api.ResidentEigenPair.from_host(api.EigenPair(values, V))


def problem(n, m, kind, binomial, seed):
    rng = np.random.default_rng(seed)
    if kind == "range":
        idx = np.arange(7, 7 + m)
    elif kind == "perm":
        idx = rng.permutation(n)[:m]
    else:                                                   # repeated rows
        idx = rng.integers(0, n, m)
        idx[m // 2:] = idx[: m - m // 2]
    N = rng.integers(1, 6, m).astype(np.float64) if binomial else np.ones(m)
    Y = rng.binomial(N.astype(int), 0.35).astype(np.float64)
    return idx, Y, N


# ---- m <= K: the dense loop of the existing entry ---------------------------------------------------------------------
@pytest.mark.parametrize("K,m,perm", [(50, 40, False), (200, 150, True), (200, 200, False), (65, 1, True)])
def test_dense_route_is_the_existing_entry(K, m, perm):
    n = 3000
    _, rp = synthetic_pair(n, 240, seed=K + m)
    idx, Y, N = problem(n, m, "perm" if perm else "range", False, K * m)
    for t, sigma in [(3.0, 1e-3), (0.5, 0.1)]:
        amll, it_ref = rp.marginal_log_likelihood_logit_la(K, t, idx, Y, N, sigma=sigma, return_iters=True)
        got, it = rp.logit_objective(t, K, idx, Y, sigma=sigma, approach="marginal", return_iters=True)
        assert it == it_ref
        assert np.float64(got).tobytes() == np.float64(-amll).tobytes(), (got, -amll)
        for prior in (None, (0.5, 3.0, 1.5)):
            post, it2 = rp.logit_objective(t, K, idx, Y, sigma=sigma, prior=prior, return_iters=True)
            ref = -amll + prior_term(t, prior or (1e-2, 10.0, 2.0))
            assert it2 == it_ref
            assert abs(post - ref) <= 1e-15 * abs(ref), (post, ref)
    rp.free()


def test_dense_route_binomial_n():
    n, K, m = 2000, 120, 100
    _, rp = synthetic_pair(n, K, seed=5)
    idx, Y, N = problem(n, m, "perm", True, 6)
    amll, it_ref = rp.marginal_log_likelihood_logit_la(K, 2.0, idx, Y, N, sigma=1e-3, return_iters=True)
    got, it = rp.logit_objective(2.0, K, idx, Y, N=N, approach="marginal", return_iters=True)
    assert it == it_ref and np.float64(got).tobytes() == np.float64(-amll).tobytes()
    rp.free()


# ---- m > K: the low-rank loop -----------------------------------------------------------------------------------------
def check_lowrank(ep, rp, K, idx, Y, N, t, sigma, dense=True):
    m = idx.size
    got, it = rp.logit_objective(t, K, idx, Y, N=N, sigma=sigma, approach="marginal", return_iters=True)
    lam = np.exp(-t * (1.0 - ep.values[:K]))
    Nn = np.ones(m) if N is None else N
    lr, it_lr = np_lowrank(np.ascontiguousarray(ep.vectors[idx, :K]), lam, sigma, Y, Nn)
    assert it == it_lr
    assert abs(got + lr) <= 1e-11 * abs(lr), (got, -lr)
    if dense:
        C = hk(ep.values, ep.vectors, K, t, idx, idx) + sigma * np.eye(m)
        ref, it_ref, L = np_amll(C, Y, Nn)
        assert it == it_ref
        # the one departure: 0.5 log det B exactly instead of sum log(L_ii + 1e-9) (include/flgp_hip.h)
        allow = 1e-10 * abs(ref) + 1e-9 * (1.0 / np.diag(L)).sum()
        assert abs(got + ref) <= allow, (got, -ref, allow)
    return got, it


@pytest.mark.parametrize("K", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("mk", ["K+1", "2K", "1000", "2500"])
def test_lowrank_against_dense(K, mk):
    m = {"K+1": K + 1, "2K": 2 * K, "1000": 1000, "2500": 2500}[mk]
    n = 4000
    ep, rp = synthetic_pair(n, 130, seed=K)
    cases = [("range", False, 0.5, 1e-3), ("perm", True, 3.0, 0.0), ("repeat", False, 3.0, 1e-3), ("perm", True, 0.5, 1e-3)]
    for c, (kind, binomial, t, sigma) in enumerate(cases):
        idx, Y, N = problem(n, m, kind, binomial, 100 * K + m + c)
        check_lowrank(ep, rp, K, idx, Y, N if binomial else None, t, sigma)
    rp.free()


def test_lowrank_posterior_adds_the_prior():
    n, K, m = 3000, 40, 500
    ep, rp = synthetic_pair(n, K, seed=8)
    idx, Y, _ = problem(n, m, "perm", False, 9)
    marg = rp.logit_objective(2.0, K, idx, Y, approach="marginal")
    for prior in (None, (0.5, 3.0, 1.5)):
        post = rp.logit_objective(2.0, K, idx, Y, prior=prior)
        ref = marg + prior_term(2.0, prior or (1e-2, 10.0, 2.0))
        assert abs(post - ref) <= 1e-15 * abs(ref)
    rp.free()


def test_lowrank_scale():
    """n = 1e6, K = 200, m = 1e5 (10 % labelled): the dense entry would need two 80 GB matrices."""
    n, K, m = 1_000_000, 200, 100_000
    ep, rp = synthetic_pair(n, K, seed=11)
    rng = np.random.default_rng(12)
    idx = np.sort(rng.choice(n, m, replace=False))
    Y = (rng.uniform(size=m) < 0.3).astype(np.float64)
    got, it = check_lowrank(ep, rp, K, idx, Y, np.ones(m), 4.0, 1e-3, dense=False)
    assert np.isfinite(got) and it >= 1
    idx_r = np.arange(n - m, n)
    check_lowrank(ep, rp, K, idx_r, Y, np.ones(m), 4.0, 1e-3, dense=False)
    rp.free()


@pytest.mark.parametrize("K,m", [(200, 150), (40, 500)], ids=["dense", "lowrank"])
def test_max_iter_is_not_an_error(K, m):
    n = 3000
    ep, rp = synthetic_pair(n, 200, seed=13)
    idx, Y, N = problem(n, m, "perm", False, 14)
    got, it = rp.logit_objective(3.0, K, idx, Y, approach="marginal", max_iter=2, return_iters=True)
    assert it == 2 and np.isfinite(got)
    C = hk(ep.values, ep.vectors, K, 3.0, idx, idx) + 1e-3 * np.eye(m)
    ref, it_ref, L = np_amll(C, Y, N, max_iter=2)
    assert it_ref == 2
    assert abs(got + ref) <= 1e-10 * abs(ref) + 1e-9 * (1.0 / np.diag(L)).sum()
    rp.free()


@pytest.mark.parametrize("K,m", [(200, 150), (40, 500)], ids=["dense", "lowrank"])
def test_determinism(K, m):
    n = 3000
    _, rp = synthetic_pair(n, 200, seed=15)
    idx, Y, N = problem(n, m, "perm", True, 16)
    a = rp.logit_objective(1.5, K, idx, Y, N=N)
    b = rp.logit_objective(1.5, K, idx, Y, N=N)
    assert np.float64(a).tobytes() == np.float64(b).tobytes()
    rp.free()


# ---- errors -----------------------------------------------------------------------------------------------------------
def test_unsupported_approach():
    _, rp = synthetic_pair(500, 20, seed=17)
    idx, Y, _ = problem(500, 30, "range", False, 18)
    for approach in ("bayes", "Marginal", ""):
        with pytest.raises(_lib.FlgpError) as e:
            rp.logit_objective(1.0, 20, idx, Y, approach=approach)
        assert e.value.code == -3 and e.value.message == "This model selection approach is not supported!"
    rp.free()


def _raw(rp, K=20, idx=None, m=30, Y=None, N=None, sigma=1e-3, approach=b"posterior", prior=None, t=1.0, max_iter=100,
         value=True):
    idx = np.arange(m, dtype=np.int32) if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
    Y = np.zeros(m) if Y is None else np.ascontiguousarray(Y, dtype=np.float64)
    v = ctypes.c_double()
    return _lib.lib().flgp_eigenpair_logit_objective(rp._h if rp is not None else None, K, idx.ctypes.data, m, Y.ctypes.data,
                                                     None if N is None else np.ascontiguousarray(N, dtype=np.float64).ctypes.data,
                                                     sigma, approach, None if prior is None else
                                                     np.ascontiguousarray(prior, dtype=np.float64).ctypes.data,
                                                     t, 1e-5, max_iter, ctypes.byref(v) if value else None, None)


def test_invalid_arguments():
    n = 500
    _, rp = synthetic_pair(n, 20, seed=19)
    L = _lib.lib()
    assert _raw(rp) == 0 and _raw(rp, approach=b"marginal", t=-1.0) == 0     # the valid baselines
    bad = {
        "null pair": dict(rp=None),
        "null value": dict(value=False),
        "K = 0": dict(K=0),
        "K > ep.K": dict(K=21),
        "m = 0": dict(m=0, idx=np.zeros(1)),
        "max_iter = 0": dict(max_iter=0),
        "row out of range": dict(idx=np.r_[np.arange(29), n]),
        "negative row": dict(idx=np.r_[-1, np.arange(29)]),
        "N = 0": dict(N=np.r_[np.ones(29), 0.0]),
        "Y > N": dict(Y=np.r_[np.zeros(29), 2.0]),
        "Y < 0": dict(Y=np.r_[np.zeros(29), -1.0]),
        "Y > 1 without N": dict(Y=np.r_[np.zeros(29), 1.5]),
        "t nan": dict(t=float("nan")),
        "t inf marginal": dict(t=float("inf"), approach=b"marginal"),
        "t = 0 posterior": dict(t=0.0),
        "t < 0 posterior": dict(t=-1.0),
        "sigma < 0": dict(sigma=-1e-3),
        "prior nan": dict(prior=[1e-2, float("nan"), 2.0]),
        "prior inf": dict(prior=[float("inf"), 10.0, 2.0]),
    }
    for name, kw in bad.items():
        kw = dict(kw)
        r = kw.pop("rp", rp)
        assert _raw(r, **kw) == -1, name
        assert L.flgp_last_error().decode(), name
    # a null approach is a null pointer, not an unsupported string
    assert _raw(rp, approach=None) == -1
    rp.free()
