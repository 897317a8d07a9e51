"""numpy restatements for the joint posterior of served rows (include/flgp_hip.h "joint posterior of served rows"),
each in the order the header states, so that the device's results can be compared bit for bit:

  cols     out(i, c) = sum_a A(i, a) P(idx(i, a), c0 + c): one chain over a ascending, multiply then add, from 0.0 -- the chain
           np_predictor.rows walks for every z and every mean column;
  streams  xi(k; g, c, t) = normal p = k of stream (g q + c) 2^32 + t under the seed (flgp_amd/synth.py);
  fold     P_draw(j, (g q + c) S + t) = P(j, g (K + q) + K + c) + acc, acc the chain over k ascending from 0.0, multiply then
           add, of P(j, g (K + q) + k) xi(k, col)."""
import numpy as np

from flgp_amd import synth


def cols(idx, val, P, c0, nc):
    idx = np.asarray(idx); val = np.asarray(val, dtype=np.float64)
    z = np.zeros((idx.shape[0], nc))
    for a in range(idx.shape[1]):                             # multiply, then add: two roundings per term
        z = z + val[:, a:a + 1] * P[idx[:, a], c0:c0 + nc]
    return z


def stream_of(g, c, t, q):
    return ((g * q + c) << 32) + t


def normals(seed, K, groups, q, S):
    """xi, K x (groups q S): column (g q + c) S + t is synth.normal(seed, stream_of(g, c, t, q), K)"""
    xi = np.zeros((K, groups * q * S))
    for gc in range(groups * q):
        for t in range(S):
            xi[:, gc * S + t] = synth.normal(seed, (gc << 32) + t, K)
    return xi


def radius(seed, K, groups, q, S):
    """sqrt(-2 log u1) of every entry of normals(): what the bound of the device's normals scales with"""
    rad = np.zeros((K, groups * q * S))
    for gc in range(groups * q):
        for t in range(S):
            rad[:, gc * S + t] = np.sqrt(-2.0 * np.log(synth.uniform(seed, (gc << 32) + t, 2 * K)[0::2]))
    return rad


def fold(P, groups, K, q, S, xi):
    """P_draw (s x groups q S) from the source operand P (s x ldp) and xi (K x groups q S)"""
    w = K + q
    out = np.zeros((P.shape[0], groups * q * S))
    for g in range(groups):
        for c in range(q):
            lo = (g * q + c) * S
            acc = np.zeros((P.shape[0], S))
            for k in range(K):
                acc = acc + P[:, g * w + k:g * w + k + 1] * xi[k:k + 1, lo:lo + S]
            out[:, lo:lo + S] = P[:, g * w + K + c:g * w + K + c + 1] + acc
    return out
