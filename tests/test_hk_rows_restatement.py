"""CPU: the numpy restatement of flgp_dev_hk_rows (tests/np_hk_rows.py) against the oracle's HK_from_spectrum on spectra
the oracle builds from small clouds, at the project's 1e-8 max|H|; and the restatement's own fma against the C library's.
What passes here gives the bit-for-bit assertions of tests/test_gpu_hk_rows.py their meaning."""
import ctypes
import ctypes.util
import math

import numpy as np
import pytest

import np_hk_rows as R
from conftest import make_case


def test_fma_is_the_c_librarys():
    """single rounding, on ordinary terms, on sums that cancel to the last bits and on exact zeros"""
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.fma.restype = ctypes.c_double
    libm.fma.argtypes = [ctypes.c_double] * 3
    rng = np.random.default_rng(11)
    N = 20000
    a = rng.normal(size=N) * 10.0 ** rng.uniform(-3, 3, N)
    b = rng.normal(size=N) * 10.0 ** rng.uniform(-3, 3, N)
    c = rng.normal(size=N) * 10.0 ** rng.uniform(-6, 6, N)
    h = N // 2
    c[:h] = -(a[:h] * b[:h]) * (1.0 + rng.integers(-3, 4, h) * 2.0 ** -52)
    c[:200] = 0.0
    a[200:300] = 0.0
    a[300:1300] = 1.0 + 2.0 ** -30 * rng.integers(1, 1000, 1000)
    b[300:1300] = 1.0 + 2.0 ** -30 * rng.integers(1, 1000, 1000)
    c[300:1300] = rng.choice([1.0, 2.0 ** 53, -2.0 ** 52, 2.0 ** -20], 1000)
    ref = np.array([libm.fma(x, y, z) for x, y, z in zip(a, b, c)])
    np.testing.assert_array_equal(R.fma(a, b, c).view(np.int64), ref.view(np.int64))
    assert np.count_nonzero(a * b + c != ref) > N // 10          # (the inputs tell a fused chain from multiply-then-add)


@pytest.mark.parametrize("n,d,s,r,K,m,t,gl,root", [
    (600, 3, 60, 5, 12, 40, 5.0, "cluster-normalized", True),
    (500, 8, 48, 10, 48, 33, 10.0, "normalized", False),       # K == s
    (257, 2, 31, 3, 7, 1, 2.0, "rw", True),
])
def test_restatement_is_hk_from_spectrum(oracle, n, d, s, r, K, m, t, gl, root):
    X, U0, U = make_case(n, d, s, r, seed=3)
    eidx, zval = oracle.cross_similarity(X, U, r, gl=gl)
    aval, _ = oracle.scale_A(eidx, zval, s)
    lam, V = np.linalg.eigh(oracle.gram(eidx, aval, s))
    lam = lam[::-1][:K].copy(); Vs = np.asfortranarray(V[:, ::-1][:, :K])
    assert lam[-1] > 1e-10 * lam[0]
    sigma = np.sqrt(lam)
    vectors = oracle.u_recover(eidx, aval, s, Vs, sigma)          # n x K: (A v / sigma) sqrt(n)
    values = sigma if root else lam
    Ho = oracle.hk_from_spectrum(values, vectors, K, t, np.arange(n, dtype=np.int32), np.arange(m, dtype=np.int32))
    H = R.hk_rows(eidx, aval, Vs, lam, math.sqrt(float(n)), values, t, vectors[:m])
    assert H.shape == Ho.shape
    assert np.abs(H - Ho).max() <= 1e-8 * np.abs(Ho).max()
    # Wm for the anchors in use is Wm: the short cut of hk_rows changes no bit
    B, q = R.b_matrix(Vs, lam, math.sqrt(float(n)))
    full = R.h_rows(eidx, aval, R.wm(B, R.vw(vectors[:m], R.weights(values, t))))
    np.testing.assert_array_equal(H, full)


def test_zero_sigma_column_contributes_nothing():
    """eig_k = 0 (and a negative one): q_k = 0, and H is bit for bit the H of the spectrum without those columns"""
    rng = np.random.default_rng(5)
    n, s, r, K, m = 50, 20, 4, 6, 9
    idx = rng.integers(0, s, size=(n, r)).astype(np.int32)
    val = rng.normal(size=(n, r))
    Vs = rng.normal(size=(s, K)); V1 = rng.normal(size=(m, K))
    eig = np.array([0.9, 0.5, 0.0, 0.3, -0.1, 0.2]); values = np.sqrt(np.maximum(eig, 0.0))
    _, q = R.b_matrix(Vs, eig, 3.0)
    assert q[2] == 0.0 and q[4] == 0.0 and (q[[0, 1, 3, 5]] > 0.0).all()
    keep = [0, 1, 3, 5]
    H = R.hk_rows(idx, val, Vs, eig, 3.0, values, 2.0, V1)
    np.testing.assert_array_equal(H, R.hk_rows(idx, val, Vs[:, keep], eig[keep], 3.0, values[keep], 2.0, V1[:, keep]))


def test_slice_width_edges():
    assert [R.slice_width(s) for s in (5120, 5121, 6826, 6827, 10240, 10241, 20480, 20481)] == [4, 3, 3, 2, 2, 1, 1, 0]
