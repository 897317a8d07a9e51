"""numpy restatements for the logit posterior on the resident pair (flgp_eigenpair_logit_posterior).

dense_*: GPML Alg. 3.1 / 3.2 on the m x m C11 as the reference writes them (posterior_distribution_classification,
src/Utils.cpp:252-299) -- the algebra of tests/test_gpu_classification.py's np_newton / np_posterior, with the step norms
of the loop returned as well.  weight_space_* / predict: the m > K route exactly as include/flgp_hip.h states it."""
import numpy as np
import scipy.linalg as sl


def lam_of(values, K, t):
    return np.exp(-t * (1.0 - values[:K]))


def hk(values, V, K, t, i0, i1):
    return (V[i0, :K] * lam_of(values, K, t)) @ V[i1, :K].T


def dense_newton(C, Y, tol=1e-5, max_iter=100):
    """Alg. 3.1 from f = 0 with N = 1; returns (f, iterations, the step norms |f - f_new|_1)."""
    m = Y.size
    f = np.zeros(m)
    steps = []
    for it in range(1, max_iter + 1):
        pi = 1.0 / (1.0 + np.exp(-f))
        W = pi * (1 - pi)
        sW = np.sqrt(W)
        L = np.linalg.cholesky(sW[:, None] * C * sW[None, :] + np.eye(m))
        b = W * f + (Y - pi)
        a = b - sW * sl.cho_solve((L, True), sW * (C @ b))
        f_new = C @ a
        steps.append(np.abs(f - f_new).sum())
        f = f_new
        if steps[-1] < tol:
            break
    return f, it, steps


def dense_posterior(values, V, K, t, idx0, idx1, Y, sigma11, sigma22, tol=1e-5, max_iter=100):
    """check_posterior's reference (tests/test_gpu_classification.py): returns (mean, cov, C22, iterations, step norms)."""
    m = idx0.size
    C11 = hk(values, V, K, t, idx0, idx0) + sigma11 * np.eye(m)
    C21 = hk(values, V, K, t, idx1, idx0)
    C22 = ((V[idx1, :K] ** 2) * lam_of(values, K, t)).sum(1) + sigma22
    f, it, steps = dense_newton(C11, Y, tol, max_iter)
    pi = 1.0 / (1.0 + np.exp(-f))
    sW = np.sqrt(pi * (1 - pi))
    B = sW[:, None] * C11 * sW[None, :] + np.eye(m)
    beta = sW[:, None] * sl.cho_solve((np.linalg.cholesky(B), True), np.eye(m)) * sW[None, :]
    mean = C21 @ (Y - pi)
    cov = C22 - ((C21 @ beta) * C21).sum(1)
    return mean, cov, C22, it, steps


def tolerances(mean, cov, C22, m):
    """check_posterior's: atol of the mean, atol of the variance (with its m / 4 allowance)."""
    return 1e-9 * np.abs(mean).max(), 1e-9 * np.abs(cov).max() + 2e-15 * C22.max() * m * 0.25


def weight_space_solve(V1, ls, f, Y, sigma11):
    """W, b, D and the factor of Q = I + X^T X at f, then beta = Q^-1 L^1/2 V1^T (b / D)."""
    pi = 1.0 / (1.0 + np.exp(-f))
    W = pi * (1 - pi)
    b = W * f + (Y - pi)
    D = 1.0 + sigma11 * W
    X = np.sqrt(W / D)[:, None] * (V1 * ls)
    LQ = np.linalg.cholesky(np.eye(ls.size) + X.T @ X)
    r = ls * (V1.T @ (b / D))
    return W, b, D, LQ, sl.cho_solve((LQ, True), r)


def weight_space_mode(values, V, K, t, idx0, Y, sigma11, tol=1e-5, max_iter=100):
    """The loop from f = 0, then the weights once more at the final f; returns (beta, L_Q, iterations, step norms)."""
    ls = np.sqrt(lam_of(values, K, t))
    V1 = V[idx0, :K]
    f = np.zeros(idx0.size)
    steps = []
    for it in range(1, max_iter + 1):
        W, b, D, _, beta = weight_space_solve(V1, ls, f, Y, sigma11)
        p = V1 @ (ls * beta)
        f_new = p + sigma11 * (b - W * p) / D
        steps.append(np.abs(f - f_new).sum())
        f = f_new
        if steps[-1] < tol:
            break
    _, _, _, LQ, beta = weight_space_solve(V1, ls, f, Y, sigma11)
    return beta, LQ, it, steps


def predict(values, V, K, t, idx1, beta, LQ, sigma22):
    """mean_i = v2_i^T L^1/2 beta, var_i = sigma22 + |L_Q^-1 L^1/2 v2_i|^2 (summed in ascending j)."""
    ls = np.sqrt(lam_of(values, K, t))
    V2 = V[idx1, :K]
    Z = sl.solve_triangular(LQ, (V2 * ls).T, lower=True)
    s = np.zeros(idx1.size)
    for j in range(K):
        s += Z[j] ** 2
    return V2 @ (ls * beta), sigma22 + s


def weight_space_posterior(values, V, K, t, idx0, idx1, Y, sigma11, sigma22, tol=1e-5, max_iter=100):
    beta, LQ, it, steps = weight_space_mode(values, V, K, t, idx0, Y, sigma11, tol, max_iter)
    mean, cov = predict(values, V, K, t, idx1, beta, LQ, sigma22)
    return mean, cov, it, steps
