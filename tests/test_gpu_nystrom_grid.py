"""GPU: the Nystrom bandwidth grid (include/flgp_hip.h ``flgp_nystrom_grid_*``) -- the anchor side once for
l bandwidths, the extension per row set.  The grid keeps the arithmetic order of the single-bandwidth entry, so its values
and extensions are compared with ``nystrom_eigenpair_cpp`` bit for bit, and with the numpy restatement at the tolerances
of ``test_gpu_parity.py::test_nystrom_eigenpair``."""
import functools
import os
import re

import numpy as np
import pytest

from flgp_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_A2S = tuple(np.exp(np.linspace(np.log(0.1), np.log(10.0), 10)))      # R/Fit.R:187-189
NARROW = (0.5, 0.7, 1.0, 1.3)
BATCH = int(re.search(r"#define\s+FLGP_NYSTROM_GRID_BATCH\s+(\d+)", open(os.path.join(ROOT, "include", "flgp_hip.h")).read()).group(1))


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()


@functools.lru_cache(maxsize=None)
def cloud(n, d, s, seed):
    """points and anchors as in test_nystrom_eigenpair"""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)); U = X[rng.permutation(n)[:s]] + 0.01 * rng.normal(size=(s, d))
    return X, U


@functools.lru_cache(maxsize=None)
def single(n, d, s, seed, a2, K, lo, hi):
    """the single-bandwidth entry on rows [lo, hi): the reference of every bit-for-bit comparison, computed once"""
    X, U = cloud(n, d, s, seed)
    ep = api.nystrom_eigenpair_cpp(X[lo:hi], U, a2, K)
    ep.values.setflags(write=False); ep.vectors.setflags(write=False)
    return ep


def row_block(s, K, z):
    """R(z) of include/flgp_hip.h: rows per block of an extension that holds z blocks of the similarity at once"""
    cap = (2 ** 28 // s) // z
    rnd = 65536 // -(-K // 128)
    rows = cap // rnd * rnd
    if rows == 0:
        rows = cap // 256 * 256
    return max(rows, 256)


SHAPES = [(700, 3, 65, 6, DEFAULT_A2S),        # one anchor chunk plus one anchor
          (900, 9, 130, 8, NARROW),
          (1500, 40, 200, 12, NARROW),         # GEMM dot route, d > 32
          (3000, 64, 257, 5, (0.7, 1.0)),      # DP = 64
          (600, 70, 96, 4, (0.7, 1.3))]        # d > 64, D_UU through the GEMM


@pytest.mark.parametrize("n,d,s,K,a2s", SHAPES)
def test_grid_equals_single_entry_bit_for_bit(n, d, s, K, a2s):
    X, U = cloud(n, d, s, n)
    m = 257
    l = len(a2s)
    for max_parallel in (1, l):
        grid = api.nystrom_spectrum_grid(U, a2s, K, max_parallel=max_parallel)
        assert (grid.s, grid.d, grid.l, grid.K) == (s, d, l, K) and 1 <= grid.workers <= max_parallel
        train = grid.extend_all(X[:m])
        assert len(train) == l
        for i, a2 in enumerate(a2s):
            ref = single(n, d, s, n, a2, K, 0, n)
            np.testing.assert_array_equal(grid.values[i], ref.values)
            ep = grid.extend(i, X)
            np.testing.assert_array_equal(ep.values, ref.values)
            np.testing.assert_array_equal(ep.vectors, ref.vectors)
            ref_m = single(n, d, s, n, a2, K, 0, m)
            np.testing.assert_array_equal(train[i].values, ref_m.values)
            np.testing.assert_array_equal(train[i].vectors, ref_m.vectors)
            # another row set from the same handle
            ref_2 = single(n, d, s, n, a2, K, n - 131, n)
            np.testing.assert_array_equal(grid.extend(i, X[n - 131:]).vectors, ref_2.vectors)
        grid.free()


@pytest.mark.parametrize("l", [1, BATCH, BATCH + 1])
@pytest.mark.parametrize("n,d,s,K", [(900, 9, 130, 8), (1500, 40, 200, 12)])      # register route and GEMM dot route
def test_batches_of_bandwidths(n, d, s, K, l):
    """l = 1, one full batch of the multi-bandwidth kernel, and a full batch followed by a batch of one"""
    X, U = cloud(n, d, s, n)
    a2s = tuple(np.linspace(0.5, 1.3, BATCH + 1)[:l])
    grid = api.nystrom_spectrum_grid(U, a2s, K, max_parallel=l)
    got = grid.extend_all(X)
    for i, a2 in enumerate(a2s):
        ref = single(n, d, s, n, a2, K, 0, n)
        np.testing.assert_array_equal(got[i].values, ref.values)
        np.testing.assert_array_equal(got[i].vectors, ref.vectors)
    grid.free()


def test_row_counts_and_row_blocks():
    """one row, 257 rows, and one row more than a row block of extend_all (whose extension GEMM must take the split-k
    plan of the single entry's block, not that of its own shrunken one)"""
    s, l, d, K = 2100, 3, 4, 12
    rows = row_block(s, K, min(l, BATCH))
    assert rows == 42496 and row_block(s, K, 1) == 65536
    n = rows + 1
    X, U = cloud(n, d, s, 5)
    a2s = (0.7, 1.0, 1.3)
    grid = api.nystrom_spectrum_grid(U, a2s, K, max_parallel=l)
    for cnt in (1, 257, n):
        got = grid.extend_all(X[:cnt])
        for i, a2 in enumerate(a2s):
            ref = single(n, d, s, 5, a2, K, 0, cnt)
            np.testing.assert_array_equal(got[i].values, ref.values)
            np.testing.assert_array_equal(got[i].vectors, ref.vectors)
    np.testing.assert_array_equal(grid.extend(1, X).vectors, single(n, d, s, 5, 1.0, K, 0, n).vectors)
    grid.free()


@pytest.mark.parametrize("n,d,s,K", [(700, 3, 65, 6), (600, 2, 64, 5)])
def test_grid_against_the_restatement(oracle, n, d, s, K):
    """every bandwidth of the default grid against oracle.np_nystrom_eigenpair: the tolerances of test_nystrom_eigenpair.
    The bound on the leading vector presumes a separated leading pair, so the cloud's seed is one for which the
    restatement itself (no device involved) has top-K relative gaps >= 2.7e-4 and lambda_K >= 1e-3 at all ten bandwidths
    -- asserted below; of the seeds 0..7 that holds for 0-3 and 7 at the first shape and for 3-7 at the second, and seed
    3 is the one test_nystrom_eigenpair uses for its s = 64 case."""
    X, U = cloud(n, d, s, 3)
    grid = api.nystrom_spectrum_grid(U, DEFAULT_A2S, K, max_parallel=len(DEFAULT_A2S))
    uu = (U * U).sum(1)
    mean = ((-2.0 * U @ U.T + uu[:, None]) + uu[None, :]).sum() / (s * s)
    np.testing.assert_allclose(grid.distances_mean, mean, rtol=1e-12, atol=0)
    for i, a2 in enumerate(DEFAULT_A2S):
        vals, vecs = oracle.np_nystrom_eigenpair(X, U, a2, K)
        ep = grid.extend(i, X)
        np.testing.assert_allclose(grid.values[i], vals, rtol=1e-10, atol=0)
        sign = np.sign(np.sum(ep.vectors * vecs, axis=0))
        err = np.max(np.abs(ep.vectors * sign - vecs), axis=0) / np.max(np.abs(vecs), axis=0)
        gap = np.minimum(np.abs(np.diff(vals, prepend=np.inf)), np.abs(np.diff(vals, append=-np.inf))) / vals[0]
        assert gap[:-1].min() >= 2.7e-4 and vals[-1] >= 1e-3, (a2, gap, vals)       # well posed at this grid point
        print(f"a2={a2:.4g}: max err x gap {np.max(err[:-1] * gap[:-1]):.3e}, leading {err[0]:.3e}, min gap {gap[:-1].min():.3e}")
        assert np.max(err[:-1] * gap[:-1]) < 1e-10, (a2, err, gap)
        assert err[0] < 1e-12, (a2, err[0])
    grid.free()


def test_resident_extension_feeds_the_consumers():
    n, d, s, K = 900, 9, 130, 8
    X, U = cloud(n, d, s, n)
    grid = api.nystrom_spectrum_grid(U, NARROW, K)
    idx = np.arange(200)
    all_res = grid.extend_all(X[:257], resident=True)
    for i, a2 in enumerate(NARROW):
        rp = grid.extend(i, X, resident=True)
        ref = api.nystrom_eigenpair_cpp(X, U, a2, K, resident=True)
        assert (rp.n, rp.K) == (n, K)
        np.testing.assert_array_equal(rp.HK_from_spectrum_cpp(K, 1.0, idx, idx), ref.HK_from_spectrum_cpp(K, 1.0, idx, idx))
        back = all_res[i].to_host()
        np.testing.assert_array_equal(back.values, single(n, d, s, n, a2, K, 0, 257).values)
        np.testing.assert_array_equal(back.vectors, single(n, d, s, n, a2, K, 0, 257).vectors)
        rp.free(); ref.free(); all_res[i].free()
    grid.free()


def test_row_shards_bit_identical():
    """pipeline.NystromPath.run_nystrom_grid: the anchor side is replicated, the extension is row-local"""
    import torch
    from flgp_amd.pipeline import HipStages, NystromPath
    path = NystromPath(HipStages("cuda:0"))
    rng = np.random.default_rng(17)
    n, d, s, K = 5000, 5, 300, 20
    a2s = (0.7, 1.0, 1.3)
    X = rng.normal(size=(n, d)); U = X[rng.permutation(n)[:s]]
    Xt = torch.from_numpy(np.ascontiguousarray(X.T)).cuda(); Ut = torch.from_numpy(np.ascontiguousarray(U.T)).cuda()
    values, whole, mean = path.run_nystrom_grid(Xt, Ut, a2s, K)
    values = values.cpu().numpy(); whole = whole.cpu().numpy()
    for i, a2 in enumerate(a2s):
        ep = api.nystrom_eigenpair_cpp(X, U, a2, K)
        np.testing.assert_array_equal(values[i], ep.values)
        np.testing.assert_array_equal(whole[i].T, ep.vectors)
    for lo, hi in [(0, 1777), (1777, 5000), (4999, 5000)]:
        v2, w2, mean2 = path.run_nystrom_grid(Xt[:, lo:hi].contiguous(), Ut, a2s, K)
        np.testing.assert_array_equal(v2.cpu().numpy(), values)
        np.testing.assert_array_equal(w2.cpu().numpy(), whole[:, :, lo:hi])
        assert mean2 == mean
        np.testing.assert_array_equal(path.extend_chosen(1, Xt[:, lo:hi].contiguous()).cpu().numpy(), whole[1][:, lo:hi])
    path.free_grid()


def test_errors_are_statuses():
    X, U = cloud(700, 3, 65, 700)
    with pytest.raises(api.FlgpError) as e:
        api.nystrom_spectrum_grid(U, (0.5, -1.0, 2.0), 6)
    assert e.value.code == -1 and e.value.message.startswith("bandwidth 1 (a2=-1): ")
    with pytest.raises(ValueError):
        api.nystrom_spectrum_grid(U[:10], (1.0,), 11)                      # K > s, refused in Python
    from flgp_amd import _lib
    import ctypes
    h = ctypes.c_void_p()
    a2 = np.array([1.0])
    U10 = np.asfortranarray(U[:10])
    rc = _lib.lib().flgp_nystrom_grid_create(U10.ctypes.data, 10, 3, a2.ctypes.data, 1, 11, 1, ctypes.byref(h))   # K > s, by the library
    assert rc == -1 and h.value is None
    rc = _lib.lib().flgp_nystrom_grid_create(U10.ctypes.data, 10, 3, a2.ctypes.data, 0, 3, 1, ctypes.byref(h))    # l = 0
    assert rc == -1 and h.value is None and "at least one bandwidth" in _lib.lib().flgp_last_error().decode()
    with pytest.raises(ValueError):
        api.nystrom_spectrum_grid(U, (), 6)
    with pytest.raises(api.FlgpError) as e:
        api.nystrom_spectrum_grid(np.tile(U[:1], (10, 1)), (1.0,), 3)      # coincident anchors: mean distance 0
    assert "anchors coincide" in e.value.message
    grid = api.nystrom_spectrum_grid(U, (0.7, 1.0), 6)
    for i in (-1, 2):
        with pytest.raises(IndexError):
            grid.extend(i, X)
        vec = np.zeros((700, 6), order="F")
        assert _lib.lib().flgp_nystrom_grid_extend(grid._h, i, X.ctypes.data, 700, None, vec.ctypes.data) == -1
        assert "outside 0..1" in _lib.lib().flgp_last_error().decode()
    with pytest.raises(ValueError):
        grid.extend(0, X[:, :2])                                           # wrong column count
    with pytest.raises(ValueError):
        grid.extend_all(np.zeros((5, 4)))
    grid.free()
    with pytest.raises(ValueError):
        grid.extend(0, X)                                                  # use after free
    with pytest.raises(ValueError):
        grid.values
