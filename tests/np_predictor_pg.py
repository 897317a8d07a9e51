"""numpy restatement of the Polya-Gamma predictor (include/flgp_hip.h "Polya-Gamma predictor"):

  u_b      = L_t (V1^T w_b)                  (K; w_b the collapsed weights of chain b at its final omega, tests/np_pg.py)
  P(:, b)  = B u_b                           (s; B the anchor side: Bq of tests/np_predictor.py, or a grid's V')
  f(i, b)  = sum_a A(i, a) P(idx(i, a), b)   (one chain over a ascending, multiply then add, from 0.0)
  pi       = 1 / (1 + exp(-f)),   y = (pi > 0.5),   label(i) = the first b with maximal pi(i, b)

`latent` is bit for bit what flgp_dev_predictor_pg_rows computes (sequential float64, two roundings per term); `link` is
the same three expressions in numpy -- its exp is numpy's, so pi agrees with the device to the bound the tests state, and
y / label are exact functions of a given pi."""
import numpy as np

import np_pg


def latent(idx, val, P, B):
    idx = np.asarray(idx); val = np.asarray(val, dtype=np.float64)
    f = np.zeros((idx.shape[0], B))
    for a in range(idx.shape[1]):                              # multiply, then add
        f = f + val[:, a:a + 1] * P[idx[:, a], :B]
    return f


def logistic(f):
    with np.errstate(over="ignore"):                           # exp(800) = inf, 1 / inf = 0: as on the device
        return 1.0 / (1.0 + np.exp(-np.asarray(f, dtype=np.float64)))


def labels_of(pi):
    """(y, label) of a given pi: exact.  np.argmax returns the first maximal entry, as Eigen's maxCoeff."""
    pi = np.asarray(pi)
    return (pi > 0.5).astype(np.float64), np.argmax(pi, axis=1).astype(np.float64)


def link(f):
    pi = logistic(f)
    return (pi,) + labels_of(pi)


def chain_u(V1, values, K, t, sigma, omega, Y):
    """u = L (V1^T w) of one chain from its final omega: w by np_pg.collapsed_w on C = V1 L V1^T + sigma I"""
    l, _ = np_pg.weights(values, K, t)
    C = V1 @ (l[:, None] * V1.T) + sigma * np.eye(V1.shape[0])
    w = np_pg.collapsed_w(omega, np.asarray(Y, dtype=np.float64) - 0.5, C)
    return l * (V1.T @ w)


def fold(Bside, U):
    """P (s x B) from the anchor side (s x K) and the chains' u (K x B)"""
    return np.asarray(Bside) @ np.asarray(U)
