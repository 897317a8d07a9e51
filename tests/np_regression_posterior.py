"""numpy restatement of the regression posterior in weight space (flgp_eigenpair_regression_posterior,
include/flgp_hip.h) for m > K, both noise models.  With V1 = vectors[idx0, :K], L = exp(-t (1 - values)), Phi = V1 L^1/2:

  "same"       c = noise + sigma,           Q = Phi^T Phi + c I,      beta = Q^-1 L^1/2 V1^T Y
  "different"  Z = diag(noise_a + sigma),   Q_d = I + Phi^T Z^-1 Phi, beta = Q_d^-1 L^1/2 V1^T Z^-1 Y
  mean = V2 L^1/2 beta
  var_i = c + |sqrt(c) L_Q^-1 L^1/2 v2_i|^2 with c = noise[0] + sigma and Q = Phi^T Phi + c I = L_Q L_Q^T

(the reference's drivers take the variance at pars = (t, noise[0]) whatever the noise model, src/Fit.cpp:77).  The variance
has no subtraction, so var >= c exactly."""
import numpy as np
import scipy.linalg as sl


def lam_of(values, K, t):
    return np.exp(-t * (1.0 - np.asarray(values, dtype=np.float64)[:K]))


def weight_space_mean(values, vectors, Y, idx0, idx1, K, t, noise, sigma):
    """noise: a scalar ("same") or one variance per row of idx0 ("different").  Returns m_new x q."""
    V1 = vectors[idx0, :K]; V2 = vectors[idx1, :K]
    Y = np.asarray(Y, dtype=np.float64).reshape(len(idx0), -1)
    ls = np.sqrt(lam_of(values, K, t))
    noise = np.asarray(noise, dtype=np.float64)
    if noise.ndim == 0:
        c = float(noise) + sigma
        Q = (ls[:, None] * (V1.T @ V1)) * ls[None, :] + c * np.eye(K)
        rhs = ls[:, None] * (V1.T @ Y)
    else:
        zinv = 1.0 / (noise + sigma)
        Q = (ls[:, None] * (V1.T @ (zinv[:, None] * V1))) * ls[None, :] + np.eye(K)
        rhs = ls[:, None] * (V1.T @ (zinv[:, None] * Y))
    beta = sl.cho_solve(sl.cho_factor(Q, lower=True), rhs)
    return V2 @ (ls[:, None] * beta)


def weight_space_variance(values, vectors, idx0, idx1, K, t, var, sigma):
    V1 = vectors[idx0, :K]; V2 = vectors[idx1, :K]
    ls = np.sqrt(lam_of(values, K, t))
    c = var + sigma
    Q = (ls[:, None] * (V1.T @ V1)) * ls[None, :] + c * np.eye(K)
    LQ = np.linalg.cholesky(Q)
    Z = sl.solve_triangular(LQ, (np.sqrt(c) * ls)[:, None] * V2.T, lower=True)       # K x m_new
    return c + (Z * Z).sum(0)
