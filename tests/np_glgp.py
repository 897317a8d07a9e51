"""numpy restatement of the GLGP spectrum step (reference src/Fit.cpp:383-449), dense and k-NN-sparsified, with
numpy.linalg.eigh as the eigensolver.  Not a test module: tests/test_glgp_restatement.py and tests/test_gpu_glgp.py import it.

Conventions (include/flgp_hip.h): ``Dt`` is n x n with COLUMN i = point i's list of squared distances to all
rows, so ``Dt[j, i]`` is entry j of list i; the selection is a stable argsort of every list (ties go to the lower row)."""
import numpy as np


def neighbours(threshold, n):
    return max(int(np.floor(threshold * n + 0.5)), 3)


def distances_t(X):
    """Dt[j, i] = |x_i|^2 - 2 x_i.x_j + |x_j|^2 (rounding differs from the device's FMA chains: feed the device's Dt where
    bits matter)."""
    X = np.asarray(X, dtype=np.float64)
    xx = (X * X).sum(axis=1)
    return (xx[None, :] - 2.0 * (X @ X.T)) + xx[:, None]


def kept_mask(Dt, r):
    """M[j, i] = point i keeps row j: the first r of a stable argsort of list i (+0.0 is added so that -0.0 sorts as 0.0)."""
    n = Dt.shape[0]
    order = np.argsort(Dt + 0.0, axis=0, kind="stable")
    M = np.zeros((n, n), dtype=bool)
    M[order[:r], np.arange(n)[None, :]] = True
    return M


def tau_jcut(Dt, r):
    """(tau, jcut) of every list: the r-th smallest value and the row of the last kept entry among those equal to it."""
    order = np.argsort(Dt + 0.0, axis=0, kind="stable")
    n = Dt.shape[0]
    tau = Dt[order[r - 1], np.arange(n)]
    M = kept_mask(Dt, r)
    jcut = np.array([np.flatnonzero(M[:, i] & (Dt[:, i] == tau[i])).max() for i in range(n)], dtype=np.int32)
    return tau, jcut


def mask_from_rule(Dt, tau, jcut):
    """the library's rule: entry j of list i is kept iff D < tau_i or (D == tau_i and j <= jcut_i)"""
    j = np.arange(Dt.shape[0])[:, None]
    return (Dt < tau[None, :]) | ((Dt == tau[None, :]) & (j <= jcut[None, :]))


def kept_sums(Dt, M):
    """sum of each list's kept entries, added one by one in ascending row order (numpy's sum is pairwise: not used)"""
    out = np.zeros(Dt.shape[1])
    for i in range(Dt.shape[1]):
        v = Dt[M[:, i], i]
        out[i] = np.cumsum(v)[-1] if v.size else 0.0
    return out


def similarity(Dt, M, inv_c, E=None):
    """Z(i, j) = (k_ij exp(-Dt[j, i] inv_c) + k_ji exp(-Dt[i, j] inv_c)) / 2; ``E`` (optional): exp(-Dt inv_c) from elsewhere"""
    if E is None:
        E = np.exp(-Dt * inv_c)
    A = np.where(M, E, 0.0)          # A[j, i] = a(i, j)
    return 0.5 * (A.T + A)


def normalise(Z):
    rs = 1.0 / (Z.sum(axis=1) + 1e-9)
    A = rs[:, None] * Z * rs[None, :]
    sd = 1.0 / np.sqrt(A.sum(axis=1) + 1e-9)
    return sd[:, None] * A * sd[None, :], sd


def spectrum(X, K, a2s, sparse=True, threshold=0.01, Dt=None, full=False):
    """The restatement.  Returns (list of (values, vectors), distances_mean, r); values are the K algebraically largest,
    descending; with ``full`` every item is (all n values descending, all vectors scaled alike)."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    if Dt is None:
        Dt = distances_t(X)
    if sparse:
        r = neighbours(threshold, n)
        M = kept_mask(Dt, r)
        mean = kept_sums(Dt, M).sum() / (n * r)
    else:
        r = n
        M = np.ones((n, n), dtype=bool)
        mean = Dt.sum() / (float(n) * n)
    out = []
    for a2 in a2s:
        Z = similarity(Dt, M, 1.0 / (a2 * mean)) if sparse else np.exp(-Dt * (1.0 / (a2 * mean)))
        W, sd = normalise(Z)
        W = 0.5 * (W + W.T)
        lam, V = np.linalg.eigh(W)
        lam, V = lam[::-1], V[:, ::-1]
        V = sd[:, None] * V
        V = np.sqrt(n) * V / (np.linalg.norm(V, axis=0) + 1e-9)[None, :]
        out.append((lam.copy(), V) if full else (lam[:K].copy(), V[:, :K]))
    return out, mean, r


def heat_kernel(values, vectors, K, t, idx0, idx1):
    """HK_from_spectrum_cpp: H = V0 diag(exp(-t (1 - values))) V1^T"""
    w = np.exp(-t * (1.0 - values[:K]))
    return (vectors[idx0, :K] * w[None, :]) @ vectors[idx1, :K].T
