"""numpy restatement of the Nystrom predictor (include/flgp_hip.h "Nystrom predictor"):

  D(i, j)  = (|x_i|^2 - 2 x_i . u_j) + |u_j|^2,       Z(i, j) = exp(-D(i, j) inv_c)
  rs_i     = sum_j Z(i, j) + 1e-9,   s1_i = sum_j Z(i, j) w_j,   f_i = (1 / rs_i) / (s1_i / rs_i + 1e-9)
  u_i      = f_i sum_j Z(i, j) V'(j, :)               (the extension's row, V' the pre-scaled anchor eigenvectors)
  P        = V' [G ; U^T]^T                           (s x (K + q): the first K columns V' G^T, the last q V' U)
  z_i      = f_i sum_j Z(i, j) P(j, :),   mean_i = z_i[K:],   var_i = c + sum_k z_i[k]^2

in the working precision ``dtype`` (np.float64, or np.longdouble for the reference of the GPU tests).  The sums are numpy's:
this is the algebra, not the device's summation order (which the header states and the forward bound of
tests/test_gpu_nystrom_predictor_rows.py covers)."""
import numpy as np


def similarity(X, U, inv_c, dtype=np.float64):
    X = np.asarray(X).astype(dtype); U = np.asarray(U).astype(dtype)
    D = ((X * X).sum(1)[:, None] - 2 * (X @ U.T)) + (U * U).sum(1)[None, :]
    return np.exp(-D * dtype(inv_c))


def row_factor(Z, w, dtype=np.float64):
    rs = Z.sum(1) + dtype(1e-9)
    inv = 1 / rs
    return inv / ((Z @ np.asarray(w).astype(dtype)) * inv + dtype(1e-9))


def extend(X, U, inv_c, w, Vp, dtype=np.float64):
    """the extension's rows u_i (n x K)"""
    Z = similarity(X, U, inv_c, dtype)
    return row_factor(Z, w, dtype)[:, None] * (Z @ np.asarray(Vp).astype(dtype))


def fold(Vp, G, U):
    """P (s x (K + q)) of one group from the pre-scaled anchor eigenvectors and the operand: G K x K, U K x q."""
    G = np.asarray(G); U = np.asarray(U).reshape(G.shape[0], -1)
    return np.hstack([Vp @ G.T, Vp @ U])


def rows(X, U, inv_c, w, P, groups, K, q, cg, dtype=np.float64):
    """mean n x (groups q), var n x groups; P s x ldp with group g in columns g (K + q) .."""
    Z = similarity(X, U, inv_c, dtype)
    f = row_factor(Z, w, dtype)
    wd = K + q
    z = f[:, None] * (Z @ np.asarray(P)[:, :groups * wd].astype(dtype))
    mean = np.hstack([z[:, g * wd + K:(g + 1) * wd] for g in range(groups)]) if q else np.zeros((X.shape[0], 0), dtype=dtype)
    var = np.stack([dtype(cg[g]) + (z[:, g * wd:g * wd + K] ** 2).sum(1) for g in range(groups)], axis=1)
    return mean, var
