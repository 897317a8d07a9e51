"""Plain numpy restatement of flgp_dev_hk_rows (flgp_amd/csrc/sparse.hip), one rounded operation at a time in the style
of np_sparse_stages.py: no `@`, no `sum()`, no `einsum`, so that numpy cannot pick a summation order of its own.

    B(j, k)  = Vs(j, k) * q_k,  q_k = scale / sigma_k,  sigma_k = sqrt(max(eig_k, 0)),  q_k = 0 where sigma_k = 0
    Vw(b, k) = w_k * V1(b, k),  w_k = exp(-t * (1 - values_k))
    Wm(j, b) = sum_k B(j, k) Vw(b, k)             one chain per element, k ascending from 0.0
    H(i, b)  = sum_a val(i, a) Wm(idx(i, a), b)   a ascending from 0.0, multiply, then add

Which chain the Wm product is: flgp_dev_hk_rows forms it with gemm_launch without a workspace (never split along k), and
`v_mfma_f64_16x16x4_f64` accumulates its four products as IEEE fused multiply-adds in ascending k starting from C
(NOTEBOOK, k1 + k2; scripts/probe_mfma_order.hip), so an element is acc = fma(B(j, k), Vw(b, k), acc) for k = 0 .. K - 1:
ONE rounding per term.  Nothing else here is fused: B, Vw and the terms of H are rounded products, and H adds each rounded
product to the sum (the library is built with -ffp-contract=off).  numpy has no fma, so `fma` below builds it from
error-free transformations; tests/test_hk_rows_restatement.py checks it against the C library's."""
import numpy as np

_SPLIT = 134217729.0          # 2^27 + 1: Veltkamp's splitter for binary64


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    t = _SPLIT * a; ah = t - (t - a); al = a - ah
    t = _SPLIT * b; bh = t - (t - b); bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """round(a * b + c) with a single rounding, elementwise on float64 arrays (Boldo and Melquiond, "Emulation of a FMA
    and correctly rounded sums", 2008): a b = p + e and p + c = s + u exactly, v = u + e rounded TO ODD, result = s + v
    rounded to nearest.  Valid away from overflow and underflow (|a b| between 2^-960 and 2^990, say), which is where
    the tests' data lie; exact zeros are fine."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64); c = np.asarray(c, dtype=np.float64)
    p, e = _two_prod(a, b)
    s, u = _two_sum(p, c)
    v, w = _two_sum(u, e)
    even = (v.view(np.int64) & 1) == 0
    v = np.where((w != 0.0) & even, np.nextafter(v, np.where(w > 0.0, np.inf, -np.inf)), v)
    return s + v


def weights(values, t):
    """w_k = exp(-t * (1 - values_k)): the expression of hk_scale_kernel.  (The device's exp and numpy's may differ in the
    last bit; the GPU test reads the device's w through flgp_dev_hk and hands it to `vw`.)"""
    return np.exp(-np.float64(t) * (1.0 - np.asarray(values, dtype=np.float64)))


def b_matrix(Vs, eig, scale):
    """B (s x K) and q (K)."""
    eig = np.asarray(eig, dtype=np.float64)
    sigma = np.sqrt(np.where(eig > 0.0, eig, 0.0))         # the kernel's `ev > 0.0 ? ev : 0.0`
    q = np.zeros_like(sigma)
    pos = sigma > 0.0
    q[pos] = np.float64(scale) / sigma[pos]
    return np.asarray(Vs, dtype=np.float64) * q[None, :], q


def vw(V1, w):
    """Vw (m x K) = V1(b, k) * w_k."""
    return np.asarray(V1, dtype=np.float64) * np.asarray(w, dtype=np.float64)[None, :]


def wm(B, Vw, rows=None):
    """Wm(j, b) for the anchors j in `rows` (default: all s): the k-ascending fma chain from 0.0."""
    B = np.asarray(B, dtype=np.float64)
    if rows is not None:
        B = B[np.asarray(rows)]
    acc = np.zeros((B.shape[0], Vw.shape[0]))
    for k in range(B.shape[1]):
        acc = fma(B[:, k, None], Vw[None, :, k], acc)
    return acc


def h_rows(idx, val, Wm):
    """H(i, b) = sum_a val(i, a) Wm(idx(i, a), b): np_sparse_stages.u_recover's loop without its epilogue."""
    idx = np.asarray(idx); val = np.asarray(val, dtype=np.float64)
    acc = np.zeros((idx.shape[0], Wm.shape[1]))
    for a in range(idx.shape[1]):
        acc = acc + val[:, a, None] * Wm[idx[:, a], :]
    return acc


def hk_rows(idx, val, Vs, eig, scale, values, t, V1, w=None):
    """flgp_dev_hk_rows as a whole (n x m).  Wm is formed for the anchors the rows name only: the others change nothing."""
    idx = np.asarray(idx)
    used, inv = np.unique(idx, return_inverse=True)
    B, _ = b_matrix(Vs, eig, scale)
    W = wm(B, vw(V1, weights(values, t) if w is None else w), rows=used)
    return h_rows(inv.reshape(idx.shape), val, W)


def slice_width(s):
    """eigen-columns per LDS slice (u_lds_width): min(4, floor(163840 / (8 s)))."""
    return min(4, 163840 // (8 * s)) if s >= 1 else 0
