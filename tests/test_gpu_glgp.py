"""GPU: the GLGP bandwidth-grid spectra (include/flgp_hip.h ``flgp_glgp_*``).  The selection and the
similarity are compared bit for bit with numpy on the same matrix; the dense route bit for bit with the Nystrom grid on
U = X_all; both routes with the numpy restatement (tests/np_glgp.py) fed the device's own distance lists, at bounds derived
from the eigensolver's residual pledge (1e-10 on a matrix of norm < 1; the sparse route's shift (W + I) / 2 doubles it).

The selection kernel has one route for every n (radix select over the list in global memory, no LDS-resident list), so
there is no size switch to straddle."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_glgp as G  # noqa: E402

from flgp_amd import _lib, api  # noqa: E402
from flgp_amd._lib import check  # noqa: E402

pytestmark = pytest.mark.gpu

DENSE_A2S = (0.1, 0.278, 0.774, 2.15)
SPARSE_A2S = (1.0, 2.2, 4.6, 10.0)
SPARSE_SHAPES = [(65, 2, 0.2, 13, 3, 0), (257, 3, 0.03, 8, 4, 2), (520, 6, 0.05, 26, 8, 1), (700, 8, 0.02, 14, 10, 2),
                 (2100, 4, 0.01, 21, 12, 1)]      # n, d, threshold, r, K, seed; the last: block-sparse products engage


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()


# ---------------------------------------------------------------- the two stages alone, on a caller's matrix
def _lists_to_device(Dt, ldd, pad):
    """column-major n x n at ldd: row i of the (n, ldd) tensor is list i; the padding holds a value that would win any
    selection if it were read"""
    import torch
    n = Dt.shape[0]
    buf = torch.full((n, ldd), pad, dtype=torch.float64, device="cuda")
    buf[:, :n] = torch.from_numpy(np.ascontiguousarray(Dt.T)).cuda()
    return buf


def dev_select(Dt, r, ldd=None):
    import torch
    n = Dt.shape[0]
    ldd = n + 3 if ldd is None else ldd
    buf = _lists_to_device(Dt, ldd, -1e300)
    tau = torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
    jcut = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    ssum = torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
    check(_lib.lib().flgp_dev_glgp_select(None, buf.data_ptr(), n, ldd, r, tau.data_ptr(), jcut.data_ptr(), ssum.data_ptr()))
    torch.cuda.synchronize()
    return tau.cpu().numpy(), jcut.cpu().numpy(), ssum.cpu().numpy()


def dev_similarity(Dt, tau, jcut, inv_c, ldd=None, ldz=None):
    import torch
    n = Dt.shape[0]
    ldd = n + 3 if ldd is None else ldd
    ldz = n + 5 if ldz is None else ldz
    buf = _lists_to_device(Dt, ldd, -1e300)
    Z = torch.full((n, ldz), np.nan, dtype=torch.float64, device="cuda")
    rs = torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
    t = torch.from_numpy(np.ascontiguousarray(tau, dtype=np.float64)).cuda()
    j = torch.from_numpy(np.ascontiguousarray(jcut, dtype=np.int32)).cuda()
    check(_lib.lib().flgp_dev_glgp_similarity(None, buf.data_ptr(), n, ldd, t.data_ptr(), j.data_ptr(), float(inv_c),
                                              Z.data_ptr(), ldz, rs.data_ptr()))
    torch.cuda.synchronize()
    Zh = Z.cpu().numpy()
    assert np.isnan(Zh[:, n:]).all()                     # nothing written past a column's n rows
    return Zh[:, :n].T.copy(), rs.cpu().numpy()          # Z[i, j]


def dev_exp(M, inv_c):
    """exp(-M inv_c) elementwise by the similarity kernel itself: on the symmetric [[0, M], [M^T, 0]] with everything kept,
    Z = (e + e) / 2 = e exactly"""
    n = M.shape[0]
    S = np.zeros((2 * n, 2 * n))
    S[:n, n:] = M
    S[n:, :n] = M.T
    Z, _ = dev_similarity(S, np.full(2 * n, np.inf), np.full(2 * n, 2 * n, dtype=np.int32), inv_c)
    return Z[:n, n:]


@functools.lru_cache(maxsize=None)
def tricky(n):
    """lists full of exact ties (quantised values, duplicated rows), with signed zeros, tiny negatives and one all-equal
    list; Dt[j, i] = entry j of list i"""
    rng = np.random.default_rng(n)
    Dt = rng.uniform(0.0, 4.0, size=(n, n))
    Dt[:, ::2] = np.round(Dt[:, ::2], 1)                 # every other list: about 41 distinct values
    for a, b in ((0, n - 1), (1, n // 2), (n // 3, n // 3 + 1)):
        Dt[b, :] = Dt[a, :]                              # duplicated rows: exact ties in EVERY list
    Dt[:, n // 2] = 2.5                                  # an all-equal list
    Dt[0, 0] = -0.0; Dt[n - 1, 0] = 0.0; Dt[n // 2, 0] = 0.0; Dt[1, 0] = -3e-17; Dt[2, 0] = -1e-300
    Dt[np.arange(n), np.arange(n)] *= rng.choice([0.0, -0.0, 1.0], size=n)      # self distances: +-0.0 or not
    Dt.setflags(write=False)
    return Dt


@pytest.mark.parametrize("n", [3, 64, 65, 257, 1025])
def test_selection_bit_for_bit(n):
    Dt = tricky(n)
    for r in sorted({min(3, n), min(8, n), n - 1, n}):
        tau, jcut, ssum = dev_select(Dt, r)
        M = G.kept_mask(Dt, r)
        want_tau, want_jcut = G.tau_jcut(Dt, r)
        np.testing.assert_array_equal(tau, want_tau)
        np.testing.assert_array_equal(jcut, want_jcut)
        np.testing.assert_array_equal(ssum, G.kept_sums(Dt, M))
        assert np.array_equal(G.mask_from_rule(Dt, tau, jcut), M)
        again = dev_select(Dt, r, ldd=n)
        for a, b in zip((tau, jcut, ssum), again):
            assert a.tobytes() == b.tobytes()            # two calls, another ldd: the same bits (the sign of a zero too)


@pytest.mark.parametrize("n", [3, 64, 65, 257, 1025])
def test_similarity_bit_for_bit(n):
    Dt = tricky(n)
    inv_c = 0.37
    E = dev_exp(Dt, inv_c)                               # E[j, i] = exp(-Dt[j, i] inv_c) in the device's exp
    ulp = np.abs(E - np.exp(-Dt * inv_c)) / np.spacing(E)
    print(f"n={n}: device exp against numpy: max {ulp.max():.0f} ulp")
    assert ulp.max() <= 2
    for r in sorted({min(3, n), min(8, n), n - 1, n}):
        M = G.kept_mask(Dt, r)
        tau, jcut = G.tau_jcut(Dt, r)
        Z, rs = dev_similarity(Dt, tau, jcut, inv_c)
        np.testing.assert_array_equal(Z, G.similarity(Dt, M, inv_c, E=E))
        np.testing.assert_array_equal(Z, Z.T)
        np.testing.assert_allclose(rs, Z.sum(axis=1), rtol=1e-13)
        Z2, rs2 = dev_similarity(Dt, tau, jcut, inv_c, ldd=n, ldz=n)
        assert Z2.tobytes() == Z.tobytes() and rs2.tobytes() == rs.tobytes()


# ---------------------------------------------------------------- the grid
@functools.lru_cache(maxsize=None)
def points(n, d, seed):
    X = np.random.default_rng(seed).normal(size=(n, d))
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def device_lists(n, d, seed):
    """the lists the grid selects from (flgp_dev_glgp_distances): Dt[j, i] = entry j of list i"""
    import torch
    X = points(n, d, seed)
    Xd = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()               # column-major n x d
    out = torch.zeros((n, n), dtype=torch.float64, device="cuda")
    check(_lib.lib().flgp_dev_glgp_distances(None, Xd.data_ptr(), n, n, d, out.data_ptr(), n))
    Dt = out.cpu().numpy().T.copy()
    Dt.setflags(write=False)
    return Dt


@functools.lru_cache(maxsize=None)
def restated(n, d, seed, K, a2s, sparse, threshold):
    """the restatement on the device's lists, all n eigenpairs, computed once"""
    return G.spectrum(points(n, d, seed), K, a2s, sparse=sparse, threshold=threshold, Dt=device_lists(n, d, seed), full=True)


@functools.lru_cache(maxsize=None)
def grid(n, d, seed, K, a2s, sparse, threshold, max_parallel=4):
    X = points(n, d, seed)
    pairs, mean, r = api.glgp_spectrum_grid(X[: n // 2], X[n // 2:], K, a2s, threshold=threshold, sparse=sparse,
                                            max_parallel=max_parallel)
    for p in pairs:
        p.values.setflags(write=False); p.vectors.setflags(write=False)
    return pairs, mean, r


def gaps(lam, K):
    """relative gap of each of the top K values to its nearer neighbour, the cut lambda_K - lambda_{K+1} included"""
    top = lam[:K + 1]
    lo = np.abs(np.diff(top))                            # K differences
    return np.minimum(np.concatenate([[np.inf], lo[:-1]]), lo) / lam[0]


def vector_error(got, want):
    sign = np.sign(np.sum(got * want, axis=0))
    return np.max(np.abs(got * sign - want), axis=0) / np.max(np.abs(want), axis=0)


def test_lists_are_the_knn_arithmetic(oracle):
    """entry j of list i is the oracle's D(i, j) = fma(-2, <x_i, x_j>, |x_i|^2) + |x_j|^2 to the bit, and the r kept ones are
    the oracle's r nearest in its order of ties"""
    n, d, seed, r = 520, 6, 1, 26
    X, Dt = points(n, d, seed), device_lists(n, d, seed)
    idx, dist = oracle.knn(X, X, r, output=True)
    tau, jcut, _ = dev_select(Dt, r)
    M = G.mask_from_rule(Dt, tau, jcut)
    assert np.array_equal(M, G.kept_mask(Dt, r))
    for i in range(n):
        assert np.array_equal(np.sort(idx[i]), np.flatnonzero(M[:, i]))
        np.testing.assert_array_equal(Dt[idx[i], i], dist[i])
    assert (Dt != Dt.T).any()                            # the two orientations do differ: the selection is pinned to one


def test_dense_route():
    n, d, K, seed = 520, 6, 8, 3
    X = points(n, d, seed)
    pairs, mean, r = grid(n, d, seed, K, DENSE_A2S, False, 0.01)
    assert r == n and len(pairs) == len(DENSE_A2S)
    ny = api.nystrom_spectrum_grid(X, DENSE_A2S, K, max_parallel=4)
    assert mean == ny.distances_mean
    ref, mean_ref, _ = restated(n, d, seed, K, DENSE_A2S, False, 0.01)
    np.testing.assert_allclose(mean, mean_ref, rtol=1e-12, atol=0)
    for i, a2 in enumerate(DENSE_A2S):
        np.testing.assert_array_equal(pairs[i].values, ny.values[i])          # the same kernels, no shift
        lam, V = ref[i]
        gap = gaps(lam, K)
        assert gap.min() >= 2.7e-4 and lam[K - 1] >= 1e-3, (a2, gap, lam[:K + 1])      # well posed at this grid point
        np.testing.assert_allclose(pairs[i].values, lam[:K], rtol=1e-10, atol=0)
        err = vector_error(pairs[i].vectors, V[:, :K])
        print(f"dense a2={a2:.4g}: max |dlam|/lam {np.max(np.abs(pairs[i].values - lam[:K]) / lam[:K]):.3e}, "
              f"max err x gap {np.max(err * gap):.3e}, min gap {gap.min():.3e}")
        assert np.max(err * gap) < 1e-10, (a2, err, gap)
        # sqrt(n) up to the reference's + 1e-9 guard, which the restatement carries too
        np.testing.assert_allclose(np.linalg.norm(pairs[i].vectors, axis=0), np.linalg.norm(V[:, :K], axis=0), rtol=1e-10)
    ny.free()


@pytest.mark.parametrize("n,d,threshold,r,K,seed", SPARSE_SHAPES)
def test_sparse_route(n, d, threshold, r, K, seed):
    pairs, mean, r_got = grid(n, d, seed, K, SPARSE_A2S, True, threshold)
    assert r_got == r == G.neighbours(threshold, n)
    ref, mean_ref, _ = restated(n, d, seed, K, SPARSE_A2S, True, threshold)
    np.testing.assert_allclose(mean, mean_ref, rtol=1e-12, atol=0)
    idx = np.arange(0, n, max(1, n // 150))
    for i, a2 in enumerate(SPARSE_A2S):
        lam, V = ref[i]
        gap = gaps(lam, K)
        assert gap.min() >= 6.8e-4, (a2, gap)                                 # well posed at this grid point
        assert lam[K - 1] > abs(lam[-1]), (a2, lam[K - 1], lam[-1])           # largest algebraic = largest magnitude
        dlam = np.max(np.abs(pairs[i].values - lam[:K]))
        err = vector_error(pairs[i].vectors, V[:, :K])
        hk = []
        for t in (1.0, 4.0):
            H = api.HK_from_spectrum_cpp(pairs[i], K, t, idx, idx)
            Hr = G.heat_kernel(lam, V, K, t, idx, idx)
            hk.append(np.max(np.abs(H - Hr)) / np.max(np.abs(Hr)))
        print(f"sparse n={n} a2={a2:.4g}: lambda_K {lam[K - 1]:.4f}, lambda_min {lam[-1]:.4f}, max |dlam| {dlam:.3e}, "
              f"max err x gap {np.max(err * gap):.3e}, min gap {gap.min():.3e}, H rel {max(hk):.3e}")
        assert np.all(np.diff(pairs[i].values) < 0)
        assert dlam <= 2e-10, (a2, pairs[i].values, lam[:K])
        assert np.max(err * gap) < 2e-10, (a2, err, gap)
        assert max(hk) <= 1e-8, (a2, hk)
        # sqrt(n) up to the reference's + 1e-9 guard, which the restatement carries too
        np.testing.assert_allclose(np.linalg.norm(pairs[i].vectors, axis=0), np.linalg.norm(V[:, :K], axis=0), rtol=1e-10)


# ---------------------------------------------------------------- plumbing
@pytest.mark.parametrize("sparse", [True, False])
def test_workers_entries_and_calls_give_the_same_bits(sparse):
    import torch
    n, d, K, seed, thr = 520, 6, 8, (1 if sparse else 3), 0.05
    a2s = SPARSE_A2S if sparse else DENSE_A2S
    l = len(a2s)
    X = points(n, d, seed)
    base, mean, r = grid(n, d, seed, K, a2s, sparse, thr)
    for mp in (1, l):                                                           # workers; a second call
        other, mean2, r2 = api.glgp_spectrum_grid(X[: n // 2], X[n // 2:], K, a2s, threshold=thr, sparse=sparse, max_parallel=mp)
        assert (mean2, r2) == (mean, r)
        for a, b in zip(base, other):
            assert a.values.tobytes() == b.values.tobytes() and a.vectors.tobytes() == b.vectors.tobytes()
    res, mean3, r3 = api.glgp_spectrum_grid(X[:100], X[100:], K, a2s, threshold=thr, sparse=sparse, resident=True)
    assert (mean3, r3) == (mean, r)
    for a, rp in zip(base, res):
        assert (rp.n, rp.K) == (n, K)
        back = rp.to_host()
        np.testing.assert_array_equal(back.values, a.values)
        np.testing.assert_array_equal(back.vectors, a.vectors)
        rp.free()
    # the device-pointer entry, X at a leading dimension of its own
    ldx = n + 9
    Xd = torch.zeros((d, ldx), dtype=torch.float64, device="cuda")
    Xd[:, :n] = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    vals = torch.zeros((l, K), dtype=torch.float64, device="cuda")
    vecs = torch.zeros((l, K, n), dtype=torch.float64, device="cuda")
    a2 = np.array(a2s)
    m4 = ctypes.c_double(); r4 = ctypes.c_int()
    check(_lib.lib().flgp_dev_glgp_spectrum_grid(None, Xd.data_ptr(), n, ldx, d, K, a2.ctypes.data, l, int(sparse), thr, 2,
                                                 vals.data_ptr(), vecs.data_ptr(), ctypes.byref(m4), ctypes.byref(r4)))
    torch.cuda.synchronize()
    assert (m4.value, r4.value) == (mean, r)
    for i, a in enumerate(base):
        np.testing.assert_array_equal(vals[i].cpu().numpy(), a.values)
        np.testing.assert_array_equal(vecs[i].cpu().numpy().T, a.vectors)
    # values alone
    only = torch.zeros((l, K), dtype=torch.float64, device="cuda")
    check(_lib.lib().flgp_dev_glgp_spectrum_grid(None, Xd.data_ptr(), n, ldx, d, K, a2.ctypes.data, l, int(sparse), thr, 1,
                                                 only.data_ptr(), None, None, None))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(only.cpu().numpy(), vals.cpu().numpy())


@pytest.mark.parametrize("m", [6, 40])                                          # both sides of m = K
def test_resident_sparse_pair_feeds_the_posteriors(m):
    n, d, K, seed, thr = 520, 6, 8, 1, 0.05
    X = points(n, d, seed)
    (rp,), _, _ = api.glgp_spectrum_grid(X[:m], X[m:], K, (2.2,), threshold=thr, resident=True)
    up = api.ResidentEigenPair.from_host(rp.to_host())
    rng = np.random.default_rng(m)
    idx0 = np.arange(m); idx1 = np.arange(m, m + 90)
    Yr = np.sin(X[:m, 0]) + 0.1 * rng.normal(size=m)
    Yc = (X[:m, 0] > 0).astype(float)
    a = rp.regression_posterior(Yr, idx0, idx1, K, (2.0, 0.05), 1e-5)
    b = up.regression_posterior(Yr, idx0, idx1, K, (2.0, 0.05), 1e-5)
    for key in ("train", "test"):
        np.testing.assert_array_equal(a["Y_pred"][key], b["Y_pred"][key])
    np.testing.assert_array_equal(a["posterior"]["cov"], b["posterior"]["cov"])
    assert np.isfinite(a["posterior"]["mean"]).all() and (a["posterior"]["cov"] > 0).all()
    c = rp.logit_posterior(idx0, idx1, K, 2.0, Yc, 1e-3, 1e-3)
    e = up.logit_posterior(idx0, idx1, K, 2.0, Yc, 1e-3, 1e-3)
    np.testing.assert_array_equal(c["mean"], e["mean"])
    np.testing.assert_array_equal(c["cov"], e["cov"])
    assert np.isfinite(c["mean"]).all() and (c["cov"] > 0).all()
    rp.free(); up.free()


def test_errors_are_statuses():
    X = points(520, 6, 1)
    with pytest.raises(api.FlgpError) as e:
        api.glgp_spectrum_grid(X[:10], X[10:], 4, (1.0, -1.0))
    assert e.value.code == -1 and e.value.message.startswith("bandwidth 1 (a2=-1): ")
    Xbad = np.array(X[:50]); Xbad[7, 2] = np.nan
    with pytest.raises(api.FlgpError, match="glgp: the input holds"):
        api.glgp_spectrum_grid(Xbad, X[50:60], 4, (1.0,))
    with pytest.raises(api.FlgpError, match="glgp: the points coincide"):
        api.glgp_spectrum_grid(np.ones((5, 3)), np.ones((4, 3)), 2, (1.0,), sparse=False)
    out = (ctypes.c_void_p * 2)(1, 1)
    Xf = np.asfortranarray(np.ones((9, 3))); a2 = np.array([1.0, 2.0])
    rc = _lib.lib().flgp_glgp_spectrum_grid(Xf.ctypes.data, 9, 3, 2, a2.ctypes.data, 2, 1, 0.4, 2, None, None,
                                            ctypes.addressof(out), None, None)
    assert rc == -1 and out[0] is None and out[1] is None                       # all handles NULL after a failure
