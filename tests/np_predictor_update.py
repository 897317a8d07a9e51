"""numpy restatements for the update of a regression handle (include/flgp_hip.h "conditioned on newly labelled
rows"), each in the order the header states:

  rows_e     e_i = [ z_i ; y_i - mean_i ]: z and mean the chain of np_predictor_draws.cols on the first K + q columns of P (a
             ascending, multiply then add, from 0.0), the residual one subtraction -- bit for bit what the kernel puts in LDS;
  gram_ld    S(k, l) = sum_i (w_i e_ik) e_il in long double from the float64 factors w_i e_ik and e_il, and sum_i |w_i e_ik e_il|:
             what the order-free bound of the kernel test is made of;
  chunks     the row ranges of the kernel's chunks (GC rows from row 0 of the call);
  fold       M = I + S[:K, :K] = L L^T, xi* = M^-1 S[:K, K:], P_mean' = P_mean + P_K xi*, P_K' = P_K L^-T (any float type);
  condition  the dense conditioning of a Gaussian on noisy observations in long double: the reference of the handle tests."""
import numpy as np

import np_predictor_draws as npd

LD = np.longdouble
GC, STEP, CT = 256, 32, 64                                   # PG_GC, PG_STEP, PG_CT of csrc/predictor_update.hip


def rows_e(idx, val, P, K, q, Y):
    E = npd.cols(idx, val, P, 0, K + q)
    if q:
        E[:, K:] = np.asarray(Y, dtype=np.float64).reshape(E.shape[0], q) - E[:, K:]
    return E


def gram_ld(E, w):
    """(S, sum of |terms|) in long double; the products' factors are the float64 values the kernel multiplies"""
    A = (np.asarray(w, dtype=np.float64)[:, None] * E).astype(LD)      # w_i e_ik rounded once, as the kernel stores it
    B = E.astype(LD)
    return A.T @ B, np.abs(A).T @ np.abs(B)


def gram_int(E, w):
    """S exactly, for integer-valued E and w: every partial sum of |terms| is an integer below 2^53, so the float64 product is
    exact in whatever order the BLAS adds"""
    E = np.asarray(E, dtype=np.float64); w = np.asarray(w, dtype=np.float64)
    assert np.array_equal(np.rint(E), E) and np.array_equal(np.rint(w), w)
    A = E * w[:, None]
    assert (np.abs(A).T @ np.abs(E)).max() < 2.0 ** 53
    return A.T @ E


def chunks(n, gc=GC):
    return [(i0, min(i0 + gc, n)) for i0 in range(0, n, gc)]


def fold(P, K, q, S, dtype=np.float64):
    """P' (s x (K + q)) from the first K + q columns of P and S ((K + q) x (K + q)), in `dtype`"""
    P = np.asarray(P)[:, :K + q].astype(dtype)
    S = np.asarray(S).astype(dtype)
    M = np.eye(K, dtype=dtype) + S[:K, :K]
    Lm = np.zeros((K, K), dtype=dtype)
    for j in range(K):
        d = M[j, j] - (Lm[j, :j] * Lm[j, :j]).sum()
        assert d > 0
        Lm[j, j] = np.sqrt(d)
        Lm[j + 1:, j] = (M[j + 1:, j] - Lm[j + 1:, :j] @ Lm[j, :j]) / Lm[j, j]
    Li = np.zeros((K, K), dtype=dtype)
    for c in range(K):                                             # L X = I, column by column
        x = np.zeros(K, dtype=dtype)
        x[c] = 1 / Lm[c, c]
        for j in range(c + 1, K):
            x[j] = -(Lm[j, c:j] @ x[c:j]) / Lm[j, j]
        Li[:, c] = x
    xi = Li.T @ (Li @ S[:K, K:])                                   # M^-1 R
    out = np.zeros((P.shape[0], K + q), dtype=dtype)
    out[:, :K] = P[:, :K] @ Li.T
    out[:, K:] = P[:, K:] + P[:, :K] @ xi
    return out


def ld_solve_spd(A, B):
    A = np.array(A, dtype=LD); n = A.shape[0]
    Lm = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = A[j, j] - (Lm[j, :j] * Lm[j, :j]).sum()
        assert d > 0
        Lm[j, j] = np.sqrt(d)
        Lm[j + 1:, j] = (A[j + 1:, j] - Lm[j + 1:, :j] @ Lm[j, :j]) / Lm[j, j]
    X = np.array(B, dtype=LD)
    for j in range(n):
        X[j] = (X[j] - Lm[j, :j] @ X[:j]) / Lm[j, j]
    for j in range(n - 1, -1, -1):
        X[j] = (X[j] - Lm[j + 1:, j] @ X[j + 1:]) / Lm[j, j]
    return X


def condition(C11, C1a, Caa, Y, d):
    """mean and covariance of the rows `a` given y = f_1 + N(0, diag(d)): C(a, 1) (C11 + diag d)^-1 Y and
    C(a, a) - C(a, 1) (C11 + diag d)^-1 C(1, a), in long double"""
    A = np.array(C11, dtype=LD) + np.diag(np.asarray(d, dtype=LD))
    sol = ld_solve_spd(A, np.hstack([np.asarray(Y, dtype=LD), np.asarray(C1a, dtype=LD)]))
    q = np.asarray(Y).shape[1]
    C1a = np.asarray(C1a, dtype=LD)
    return C1a.T @ sol[:, :q], np.asarray(Caa, dtype=LD) - C1a.T @ sol[:, q:]
