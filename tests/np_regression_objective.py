"""numpy restatement of train_regression_gp_cpp's four objectives (reference src/train.cpp:333-555), written densely as
the reference writes them: C^-1 from a Cholesky solve against the identity, explicit U and G, the reference's clipping,
then the prior terms.  Shared by tests/test_regression_objective_args.py and tests/test_gpu_regression_objective.py."""
import numpy as np
import scipy.linalg as sl

PRIOR = (1.0, 10.0, 2.0, 0.1, 1e-3)      # PostOFDataReg: p, q, tau, alpha, beta (src/train.h:153-155)


def _clip(g, thr):
    return np.where(np.abs(g) >= thr, np.sign(g) * thr, g)


def nmll(values, V_all, K, idx, Y, x, sigma, noise="same", clip=True):
    """negative_marginal_likelihood{,_diff_noise}_regression_cpp: (value, grad).  clip=False leaves the gradient
    unclipped (the exact derivative of the value)."""
    idx = np.asarray(idx)
    Y = np.asarray(Y, dtype=np.float64).reshape(idx.size, -1)
    x = np.asarray(x, dtype=np.float64)
    m, q = Y.shape
    t = x[0]
    lam = 1.0 - values[:K]
    V = V_all[idx, :K]
    A = -lam * np.exp(-t * lam)
    grad = np.zeros(x.size)
    diff = noise == "different"
    if m <= K:
        C = (V * np.exp(-t * lam)) @ V.T
        C = C + sigma * np.eye(m) + (np.diag(x[1:]) if diff else x[1] * np.eye(m))
        L = np.linalg.cholesky(C)
        alpha = sl.cho_solve((L, True), Y)
        Cinv = sl.cho_solve((L, True), np.eye(m))
        U = alpha @ alpha.T / q - Cinv
        G = (V * A) @ V.T
        grad[0] = -0.5 * (U * G.T).sum()
        if diff:
            grad[1:] = -0.5 * np.diag(U)
        else:
            grad[1] = -0.5 * np.trace(U)
            if clip:
                grad[1] = _clip(grad[1], 10.0)
        value = 0.5 * (Y * alpha).sum() / q + np.log(np.diag(L) + 1e-9).sum()
        return value, grad
    Ls = np.exp(-0.5 * t * lam) + 0.0
    if not diff:
        c = x[1] + sigma
        VtV = V.T @ V
        Q = Ls[:, None] * VtV * Ls[None, :] + c * np.eye(K)
        LQ = np.linalg.cholesky(Q)
        alpha = (Y - V @ (Ls[:, None] * sl.cho_solve((LQ, True), Ls[:, None] * (V.T @ Y)))) / c
        Qinv = sl.cho_solve((LQ, True), np.eye(K))
        Vta = V.T @ alpha
        grad[0] = -0.5 * (Vta * (A[:, None] * Vta)).sum() / q
        grad[0] += 0.5 / c * np.trace(A[:, None] * VtV)
        grad[0] += -0.5 / c * ((Qinv @ (Ls[:, None] * VtV)) * (A[:, None] * VtV * Ls[None, :]).T).sum()
        grad[1] = -0.5 * (alpha * alpha).sum() / q
        grad[1] += 0.5 / c * (m - (Qinv * (Ls[:, None] * VtV * Ls[None, :]).T).sum())
        if clip:
            grad[1] = _clip(grad[1], 10.0)
        value = 0.5 * (Y * alpha).sum() / q + np.log(np.diag(LQ) + 1e-9).sum() + 0.5 * (m - K) * np.log(c)
        return value, grad
    z = x[1:] + sigma
    zi = 1.0 / z
    VtZiV = V.T @ (zi[:, None] * V)
    Q = Ls[:, None] * VtZiV * Ls[None, :] + np.eye(K)
    LQ = np.linalg.cholesky(Q)
    alpha = zi[:, None] * Y - zi[:, None] * (V @ (Ls[:, None] * sl.cho_solve((LQ, True), Ls[:, None] * (V.T @ (zi[:, None] * Y)))))
    Qinv = sl.cho_solve((LQ, True), np.eye(K))
    grad[0] = -0.5 * (alpha * (((alpha.T @ V) * A[None, :]) @ V.T).T).sum() / q
    grad[0] += 0.5 * np.trace(A[:, None] * VtZiV)
    grad[0] += -0.5 * ((Qinv @ (Ls[:, None] * VtZiV)) * (A[:, None] * VtZiV * Ls[None, :]).T).sum()
    tmp = zi[:, None] * V * Ls[None, :]
    g = -0.5 * (alpha * alpha).sum(1) / q + 0.5 * (zi - ((tmp @ Qinv) * tmp).sum(1))
    grad[1:] = _clip(g, 1.0) if clip else g
    value = 0.5 * (Y * alpha).sum() / q + np.log(np.diag(LQ) + 1e-9).sum() + 0.5 * np.log(z + 1e-9).sum()
    return value, grad


def objective(values, V_all, K, idx, Y, x, sigma, noise="same", approach="posterior", prior=None, clip=True):
    """The objective the optimiser sees: nmll for "marginal", nmll + prior for "posterior" (src/train.cpp:333-348,
    438-457; the prior gradients are added after the clipping)."""
    if noise not in ("same", "different"):
        raise ValueError("The noise setting is illegal!")
    if approach not in ("marginal", "posterior"):
        raise ValueError("This model selection approach is not supported!")
    value, grad = nmll(values, V_all, K, idx, Y, x, sigma, noise, clip)
    if approach == "marginal":
        return value, grad
    p, pq, tau, a, b = PRIOR if prior is None else prior
    x = np.asarray(x, dtype=np.float64)
    t = x[0]
    pr0 = p * np.log(t + 1e-9) + (t / tau) ** (-pq)
    grad[0] += p / (t + 1e-9) - (pq / tau) * (t / tau) ** (-pq - 1)
    z = x[1:] + sigma
    if noise == "same":
        pr1 = (a + 1) * np.log(z[0]) + b / z[0]
        grad[1] += (a + 1) / z[0] - b / z[0] ** 2
    else:
        m = z.size
        pr1 = (((a + 1) * np.log(z) + b / z) / m).sum()
        grad[1:] += ((a + 1) / z - b / z ** 2) / m
    return value + pr0 + pr1, grad


def synthetic_pair(n, K, rng):
    """Orthonormal V (n x K, QR of a Gaussian) times sqrt(n), as the reference's vectors, and values in (0, 1]."""
    V, _ = np.linalg.qr(rng.standard_normal((n, K)))
    values = np.sort(rng.uniform(0.05, 1.0, K))[::-1].copy()
    values[0] = 1.0
    return values, np.asfortranarray(V * np.sqrt(n))


def central_diff(f, x, h):
    """(f(x + h e_i) - f(x - h e_i)) / 2h for every i, h relative to |x_i|"""
    x = np.asarray(x, dtype=np.float64)
    g = np.zeros(x.size)
    for i in range(x.size):
        hi = h * max(abs(x[i]), 1e-3)
        xp = x.copy(); xm = x.copy()
        xp[i] += hi; xm[i] -= hi
        g[i] = (f(xp) - f(xm)) / (2 * hi)
    return g
