"""numpy restatements for the greedy variance design (include/flgp_hip.h "which rows to label next"), each sum
in the order the header states:

  lane_sum    the order of predictor_rows_kernel's `sq` and of the projection: lane l adds the terms k = l, l + 64, .. ascending
              from 0.0, then six butterfly steps S_l <- S_l + S_(l xor o), o = 32, 16, 8, 4, 2, 1;
  scores0     |z_i|^2 in that order, z the chain of np_predictor_draws.cols (a ascending, multiply then add, from 0.0);
  better      the total order of the argmax: the larger score, a NaN below every number, at equal scores the lower index;
  design      the loop: picks, gain, the final scores (and, on request, the scores before every pick);
  cond_var    the dense reference in long double: |z_i|^2 - k_i^T (Z_J Z_J^T + d I)^-1 k_i through a Cholesky factor, with the
              weights alpha_i = (Z_J Z_J^T + d I)^-1 k_i the bound is made of;
  bound       the operation-count bound of DESIGN f-25 on |score - score_ld|."""
import numpy as np

import np_predictor_draws as npd

LD = np.longdouble
U53 = 2.0 ** -53


def lane_sum(terms):
    """terms (..., K) -> (...): 64 lane-strided partial sums from 0.0, then the butterfly"""
    terms = np.asarray(terms, dtype=np.float64)
    K = terms.shape[-1]
    S = np.zeros(terms.shape[:-1] + (64,))
    for c in range(0, K, 64):
        w = min(64, K - c)
        S[..., :w] = S[..., :w] + terms[..., c:c + w]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        S = S + S[..., lanes ^ o]
    return S[..., 0]


def scores0(idx, val, P, K):
    Z = npd.cols(idx, val, P, 0, K)
    return lane_sum(Z * Z)


def argbest(score, taken):
    """the lowest index among the untaken rows of maximal score; a NaN is never larger (a NaN is picked only when nothing else is
    left, the lowest index first)"""
    free = ~taken
    ok = free & ~np.isnan(score)
    if ok.any():
        top = score[ok].max()
        return int(np.flatnonzero(ok & (score == top))[0])
    return int(np.flatnonzero(free)[0])


def design(idx, val, P, K, d, B, trace=False):
    """(picks int32 B, gain B, score n[, the scores before every pick B x n]) of n ELL rows (idx, val: n x r) on the operand P"""
    idx = np.asarray(idx); val = np.asarray(val, dtype=np.float64); P = np.asarray(P, dtype=np.float64)
    n = idx.shape[0]
    PK = P[:, :K]
    score = scores0(idx, val, P, K)
    taken = np.zeros(n, dtype=bool)
    picks, gain = np.zeros(B, dtype=np.int32), np.zeros(B)
    U = np.zeros((B, K))
    before = np.zeros((B, n)) if trace else None
    for t in range(B):
        if trace:
            before[t] = score
        j = argbest(score, taken)
        picks[t], gain[t], taken[j] = j, score[j], True
        z = npd.cols(idx[j:j + 1], val[j:j + 1], P, 0, K)[0]
        b = np.zeros(t)
        for k in range(K):                                    # b_tau: k ascending, multiply then add, from 0.0
            b = b + U[:t, k] * z[k]
        acc = np.zeros(K)
        for tau in range(t):                                  # tau ascending, multiply then add, from 0.0
            acc = acc + U[tau] * b[tau]
        with np.errstate(invalid="ignore", divide="ignore"):
            u = (z - acc) / np.sqrt(gain[t] + d)
        U[t] = u
        p = lane_sum(PK * u[None, :])
        c = np.zeros(n)
        for a in range(idx.shape[1]):                         # a ascending, multiply then add, from 0.0
            c = c + val[:, a] * p[idx[:, a]]
        score = score - c * c
    return (picks, gain, score, before) if trace else (picks, gain, score)


def ld_chol(A):
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    Lm = np.zeros((n, n), dtype=LD)
    for j in range(n):
        dj = A[j, j] - (Lm[j, :j] * Lm[j, :j]).sum()
        assert dj > 0
        Lm[j, j] = np.sqrt(dj)
        if j + 1 < n:
            Lm[j + 1:, j] = (A[j + 1:, j] - Lm[j + 1:, :j] @ Lm[j, :j]) / Lm[j, j]
    return Lm


def cond_var(Z, J, d, Kx=None):
    """(var n, alpha t x n) in long double: the latent variance of every row of Z given noisy observations (variance d) of the
    rows J, var_i = |z_i|^2 - k_i . alpha_i with k_i = Z_J z_i and alpha_i = (Z_J Z_J^T + d I)^-1 k_i.  Kx: Z_J Z^T (t x n, long
    double) where the caller has it already"""
    Z = np.asarray(Z).astype(LD)
    J = np.asarray(J, dtype=np.int64)
    t = J.size
    prior = (Z * Z).sum(1)
    if t == 0:
        return prior, np.zeros((0, Z.shape[0]), dtype=LD)
    ZJ = Z[J]
    if Kx is None:
        Kx = ZJ @ Z.T
    Lm = ld_chol(Kx[:, J] + LD(d) * np.eye(t, dtype=LD))
    X = np.array(Kx)
    for j in range(t):
        X[j] = (X[j] - Lm[j, :j] @ X[:j]) / Lm[j, j]
    for j in range(t - 1, -1, -1):
        X[j] = (X[j] - Lm[j + 1:, j] @ X[j + 1:]) / Lm[j, j]
    return prior - (Kx * X).sum(0), X


def bound(absZ, J, alpha, d, K, r):
    """DESIGN f-25: |score_i - score_ld_i| <= 2^-53 [ (ceil(K / 64) + t + 8) N_i^2 + 2 G_k N_i S_i + G_G S_i^2 ] to first order,
    with t = len(J) picks, N_i^2 = |zabs_i|^2 + d on the absolute features zabs_i(k) = sum_a |A(i, a)| |P(idx(i, a), k)|,
    S_i = sum_tau |alpha_i(tau)| N_(j_tau), g1 = 2 r + ceil(K / 64) + 9, G_k = (t + 2 + g1) sqrt(t + 1) and
    G_G = (2 K + 2 g1 + t + 2) sqrt(t) + t + ceil(K / 64) + 11.  absZ: n x K; alpha: t x n (cond_var)"""
    absZ = np.asarray(absZ).astype(LD)
    t = len(J)
    N = np.sqrt((absZ * absZ).sum(1) + LD(d))
    lanes = -(-K // 64)
    g1 = 2 * r + lanes + 9
    Gk = (t + 2 + g1) * np.sqrt(LD(t + 1))
    GG = (2 * K + 2 * g1 + t + 2) * np.sqrt(LD(t)) + t + lanes + 11
    S = (np.abs(np.asarray(alpha).astype(LD)) * N[np.asarray(J, dtype=np.int64)][:, None]).sum(0) if t else np.zeros(absZ.shape[0], dtype=LD)
    return LD(U53) * ((lanes + t + 8) * N * N + 2 * Gk * N * S + GG * S * S)
