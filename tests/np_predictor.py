"""numpy restatement of the fitted predictor (include/flgp_hip.h "fitted predictor"):

  Bq(j, k) = Vs(j, k) sqrt(n_fit) / sigma_k   (sigma_k = sqrt(max(eig_k, 0)), 0 where sigma_k = 0)
  P        = Bq [G ; U^T]^T                    (s x (K + q): the first K columns Bq G^T, the last q Bq U)
  z_i      = a_i P                             (r rows of P, weighted and added)
  mean_i   = z_i[K:],   var_i = c + sum_k z_i[k]^2

and of flgp_dev_predictor_rows in the order its header states: every z is one chain over a ascending, multiply then add,
from 0.0; the squares are added per lane l = k mod 64 in k-ascending order from 0.0, then six butterfly steps
S_l <- S_l + S_(l xor o), o = 32 .. 1, and var = cg + S_0."""
import numpy as np


def anchor_side(V, eig, n_fit, K):
    ev = np.maximum(np.asarray(eig, dtype=np.float64)[:K], 0.0)
    sigma = np.sqrt(ev)
    scale = np.sqrt(float(n_fit))
    qk = np.zeros(K)
    nz = sigma > 0.0
    qk[nz] = scale / sigma[nz]
    return np.asarray(V, dtype=np.float64)[:, :K] * qk[None, :]


def fold(V, eig, n_fit, G, U):
    """P (s x (K + q)) of one group from the model's anchor side and the operand: G K x K, U K x q."""
    G = np.asarray(G, dtype=np.float64); U = np.asarray(U, dtype=np.float64).reshape(G.shape[0], -1)
    Bq = anchor_side(V, eig, n_fit, G.shape[0])
    return np.hstack([Bq @ G.T, Bq @ U])


def rows(idx, val, P, groups, K, q, cg):
    """The row kernel: idx / val n x r, P s x ldp (group g in columns g (K + q) ..).  Returns mean n x (groups q) and
    var n x groups, bit for bit what the device computes."""
    idx = np.asarray(idx); val = np.asarray(val, dtype=np.float64)
    n, r = idx.shape
    w = K + q
    mean = np.zeros((n, groups * q)); var = np.zeros((n, groups))
    lane = np.arange(64)
    for g in range(groups):
        z = np.zeros((n, w))
        for a in range(r):                                    # multiply, then add: two roundings per term
            z = z + val[:, a:a + 1] * P[idx[:, a], g * w:(g + 1) * w]
        mean[:, g * q:(g + 1) * q] = z[:, K:]
        S = np.zeros((n, 64))
        for k0 in range(0, K, 64):
            blk = z[:, k0:min(k0 + 64, K)]
            S[:, :blk.shape[1]] = S[:, :blk.shape[1]] + blk * blk
        for o in (32, 16, 8, 4, 2, 1):
            S = S + S[:, lane ^ o]
        var[:, g] = cg[g] + S[:, 0]
    return mean, var
