"""What tests/test_gpu_predictor_draws.py and tests/test_gpu_predictor_covariance.py share: the fits of tests/test_gpu_predictor.py
("A": n 3000, d 3, s 200, r 5, K 20; "As": K = s = 200; kernels "lae" and "se") and the Nystrom grid of
tests/test_gpu_nystrom_predictor.py ("s200": n 1500, d 40, s 200, K 12, a2 in (0.7, 1.0)), each made once per process and left
unchanged; the training problems of those tests; a served row's ELL weights from the stage entries the model itself runs; and
the long-double algebra of the dense references."""
import functools

import numpy as np

import np_logit_posterior as nlp
from conftest import make_case
from flgp_amd import _lib, api, synth

DEV = "cuda:0"
LD = np.longdouble
EPS = LD(2.0) ** -53
SHAPES = {"A": (3000, 3, 200, 5, 20), "As": (3000, 3, 200, 5, 200)}
EPSILON = 0.7
T, NOISE, SIGMA = 2.0, 0.1, 1e-3
NY = (1500, 40, 200, 12)
A2S = (0.7, 1.0)
NEWTON_TOL = 1e-10                                           # both sides run Newton to convergence: the mode is the mode


@functools.lru_cache(maxsize=None)
def case(shape):
    n, d, s, r, K = SHAPES[shape]
    X, U0, U = make_case(n, d, s, r, seed=n + d)
    for a in (X, U0, U):
        a.setflags(write=False)
    return X, U0, U


@functools.lru_cache(maxsize=None)
def fitted(shape, kernel="lae"):
    """(model, pair, the pair on the host)"""
    n, d, s, r, K = SHAPES[shape]
    X, U0, U = case(shape)
    model, pair = api.heat_kernel_spectrum_model(X, X[:0], s, r, K, models={"kernel": kernel, "gl": "cluster-normalized", "root": True},
                                                 epsilon=EPSILON, U=U)
    host = pair.to_host()
    host.values.setflags(write=False); host.vectors.setflags(write=False)
    return model, pair, host


def new_rows(shape, count, seed=1000):
    n, d = SHAPES[shape][:2]
    return np.asfortranarray(synth.gaussian_mixture(count, d, components=5, seed=n + d + seed))     # another draw: no fit row


def training(X, m, q, seed):
    rng = np.random.default_rng(seed)
    idx0 = rng.permutation(X.shape[0])[:m].astype(np.int32)
    Y = np.asfortranarray(np.sin(2.0 * X[idx0, :1] + np.arange(q)[None, :]) + 0.1 * rng.normal(size=(m, q)))
    return idx0, Y


def logit_problem(X, m, seed=21):
    idx0 = np.random.default_rng(seed).permutation(X.shape[0])[:m].astype(np.int32)
    Y = np.asfortranarray(np.stack([(X[idx0, 0] > np.median(X[idx0, 0])).astype(float),
                                    (X[idx0, 1] > np.median(X[idx0, 1])).astype(float)], axis=1))
    return idx0, Y, np.array([0, 1, 1], dtype=np.int32), np.array([1.5, 1.5, 4.0])    # two columns, one of them at two t


@functools.lru_cache(maxsize=None)
def ny_cloud():
    n, d, s, K = NY
    rng = np.random.default_rng(n)
    X = rng.normal(size=(n, d)); U = X[rng.permutation(n)[:s]] + 0.01 * rng.normal(size=(s, d))
    X2 = np.random.default_rng(n + 1000).normal(size=(600, d))
    for a in (X, U, X2):
        a.setflags(write=False)
    return X, U, X2


@functools.lru_cache(maxsize=None)
def ny_fitted():
    """(grid, per bandwidth the resident pair of the fit rows)"""
    X, U, X2 = ny_cloud()
    grid = api.nystrom_spectrum_grid(U, A2S, NY[3], max_parallel=len(A2S))
    return grid, [grid.extend(i, X, resident=True) for i in range(len(A2S))]


def model_ell_rows(shape, kernel, X):
    """the scaled anchor weights (idx n x r, val n x r) of the rows X under the fitted model: k-NN, LAE or SE weights and
    flgp_dev_extend_scale under the fit's sums, on the stage entries the model's own row chain runs"""
    import torch
    n_fit, d, s, r, K = SHAPES[shape]
    U0 = case(shape)[1]
    model = fitted(shape, kernel)[0]
    h = model.to_host()
    L = _lib.lib()
    n = X.shape[0]
    dev = lambda a: torch.from_numpy(np.array(a, order="C")).to(DEV)
    dX, dU = dev(np.asarray(X).T), dev(np.asarray(U0).T)
    rows, dpad = L.flgp_dev_anchor_rows(s), L.flgp_dev_anchor_dpad(d)
    dUt = torch.zeros(rows * dpad, dtype=torch.float64, device=DEV); duu = torch.zeros(rows, dtype=torch.float64, device=DEV)
    _lib.check(L.flgp_dev_anchor_prep(None, dU.data_ptr(), s, s, d, dUt.data_ptr(), duu.data_ptr()))
    knn = torch.zeros((n, r), dtype=torch.int32, device=DEV); dist = torch.zeros((n, r), dtype=torch.float64, device=DEV)
    idx = torch.zeros((n, r), dtype=torch.int32, device=DEV); val = torch.zeros((n, r), dtype=torch.float64, device=DEV)
    _lib.check(L.flgp_dev_knn(None, dX.data_ptr(), n, n, d, dUt.data_ptr(), duu.data_ptr(), s, r, knn.data_ptr(),
                              dist.data_ptr() if kernel == "se" else None, n))
    if kernel == "se":
        _lib.check(L.flgp_dev_se_weights(None, knn.data_ptr(), dist.data_ptr(), n, n, r, EPSILON, idx.data_ptr(), val.data_ptr()))
    else:
        _lib.check(L.flgp_dev_lae(None, dX.data_ptr(), n, n, d, dUt.data_ptr(), s, r, knn.data_ptr(), n, idx.data_ptr(), val.data_ptr()))
    c1, c2, sz = dev(h["colsum_gl"]), dev(h["colsum_spectrum"]), dev(h["sizes"])
    _lib.check(L.flgp_dev_extend_scale(None, idx.data_ptr(), val.data_ptr(), n, r, c1.data_ptr(), sz.data_ptr(), c2.data_ptr()))
    torch.cuda.synchronize()
    return idx.cpu().numpy(), val.cpu().numpy()


# ---- long-double algebra
def ld_chol(A):
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    Lm = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = A[j, j] - (Lm[j, :j] * Lm[j, :j]).sum()
        assert d > 0
        Lm[j, j] = np.sqrt(d)
        if j + 1 < n:
            Lm[j + 1:, j] = (A[j + 1:, j] - Lm[j + 1:, :j] @ Lm[j, :j]) / Lm[j, j]
    return Lm


def ld_spd_solve(A, B):
    """A^-1 B in long double through a Cholesky factor"""
    Lm = ld_chol(A)
    n = Lm.shape[0]
    Y = np.array(B, dtype=LD)
    for j in range(n):
        Y[j] = (Y[j] - Lm[j, :j] @ Y[:j]) / Lm[j, j]
    for j in range(n - 1, -1, -1):
        Y[j] = (Y[j] - Lm[j + 1:, j] @ Y[j + 1:]) / Lm[j, j]
    return Y


def prior_block(values, Ua, Ub, K, t):
    lam = np.exp(-LD(t) * (1 - np.asarray(values[:K]).astype(LD)))
    return (np.asarray(Ua)[:, :K].astype(LD) * lam) @ np.asarray(Ub)[:, :K].astype(LD).T


def regression_cov(values, U1, Ua, Ub, K, t, c):
    """C(a, b) - C(a, 1) (C(1, 1) + c I)^-1 C(1, b) in long double; also the largest prior diagonal of a"""
    C11 = prior_block(values, U1, U1, K, t) + LD(c) * np.eye(U1.shape[0], dtype=LD)
    Ca1, C1b = prior_block(values, Ua, U1, K, t), prior_block(values, U1, Ub, K, t)
    Cab = prior_block(values, Ua, Ub, K, t)
    return Cab - Ca1 @ ld_spd_solve(C11, C1b), float(np.diag(prior_block(values, Ua, Ua, K, t)).max())


def logit_cov(values, U1, Ua, Ub, K, t, y, sigma11):
    """C(a, b) - C(a, 1) W^1/2 B^-1 W^1/2 C(1, b), B = I + W^1/2 C11 W^1/2 with sigma11 on C11, at the mode of the restatement's
    Newton iteration (tests/np_logit_posterior.py) run to convergence; the rest in long double"""
    m = U1.shape[0]
    C11 = prior_block(values, U1, U1, K, t) + LD(sigma11) * np.eye(m, dtype=LD)
    f, it, steps = nlp.dense_newton(C11.astype(np.float64), y, tol=1e-12, max_iter=200)
    assert it < 200
    pi = 1 / (1 + np.exp(-f.astype(LD)))
    sW = np.sqrt(pi * (1 - pi))
    B = sW[:, None] * C11 * sW[None, :] + np.eye(m, dtype=LD)
    Ca1, C1b = prior_block(values, Ua, U1, K, t), prior_block(values, U1, Ub, K, t)
    Cab = prior_block(values, Ua, Ub, K, t)
    return Cab - (Ca1 * sW[None, :]) @ ld_spd_solve(B, sW[:, None] * C1b), float(np.diag(prior_block(values, Ua, Ua, K, t)).max())
