"""GPU (-m gpu): the Polya-Gamma predictor over one bandwidth of a Nystrom grid (include/flgp_hip.h) on the
clouds of tests/test_gpu_nystrom_grid.py -- (n, d, s, K) = (900, 9, 130, 8) and (1500, 40, 200, 12), a2 in (0.7, 1.0) -- one grid
and one training pair per shape, made once per module.  N_sample = 8; m = 60 > K and m = 10 <= K = 12; B = 3 (the third chain a
duplicate of the first) and B = 9 (two passes of 8 mean columns).

* against grid.extend(i, training rows stacked on 300 new rows, resident) + test_pgbinary_batch(.., sigma_nv=0), with tol_pi and
  the label condition of tests/test_gpu_predictor_pg.py (tests/predictor_pg_checks.py); omega and f are that entry's bit for bit;
* bits: 513 rows as one call, in blocks of 256 and one at a time; nystrom_dot_gemm 0 against 1 at d = 9 and d = 40; the host
  against the device entry; the existing apply returns the latent;
* a pair from another bandwidth is refused, and the bandwidth index comes before the chains' refusals."""
import functools

import numpy as np
import pytest

from flgp_amd import _lib, api
from predictor_pg_checks import compare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = {"s130": (900, 9, 130, 8), "s200": (1500, 40, 200, 12)}
A2S = (0.7, 1.0)
SIGMA, NS, NEW = 1e-2, 8, 300
CHAINS = {3: (np.array([1.5, 4.0, 1.5]), np.array([0, 1, 0], dtype=np.int32), [901, 902, 901], ((0, 2),)),
          9: (np.array([1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 4.5, 5.0]), np.array([0, 1, 0, 1, 0, 1, 0, 1, 0], dtype=np.int32),
              list(range(700, 709)), ())}


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()


@functools.lru_cache(maxsize=None)
def cloud(shape):
    """points and anchors as tests/test_gpu_nystrom_grid.py draws them, and NEW rows of another draw"""
    n, d, s, K = SHAPES[shape]
    rng = np.random.default_rng(n)
    X = rng.normal(size=(n, d)); U = X[rng.permutation(n)[:s]] + 0.01 * rng.normal(size=(s, d))
    X2 = np.random.default_rng(n + 1000).normal(size=(NEW, d))
    for a in (X, U, X2):
        a.setflags(write=False)
    return X, U, X2


@functools.lru_cache(maxsize=None)
def grid_of(shape):
    X, U, X2 = cloud(shape)
    return api.nystrom_spectrum_grid(U, A2S, SHAPES[shape][3], max_parallel=len(A2S))


def problem(shape, m, seed=21):
    X = cloud(shape)[0]
    idx0 = np.random.default_rng(seed).permutation(SHAPES[shape][0])[:m].astype(np.int32)
    Y = np.asfortranarray(np.stack([(X[idx0, 0] > np.median(X[idx0, 0])).astype(float),
                                    (X[idx0, 1] > np.median(X[idx0, 1])).astype(float)], axis=1))
    return idx0, Y


def make(grid, i, pair, idx0, K, Y, B, **kw):
    ts, col, seeds, _ = CHAINS[B]
    return api.Predictor.nystrom_pg(grid, i, pair, idx0, K, ts, Y, SIGMA, col=col, seeds=seeds, N_sample=NS, **kw)


@pytest.mark.parametrize("shape,i,m,B", [("s130", 0, 60, 3), ("s130", 1, 60, 9), ("s200", 1, 10, 3), ("s200", 0, 10, 9), ("s200", 0, 60, 9)])
def test_against_the_extension_route(shape, i, m, B):
    n, d, s, K = SHAPES[shape]
    X, U, X2 = cloud(shape)
    grid = grid_of(shape)
    idx0, Y = problem(shape, m)
    ts, col, seeds, dup = CHAINS[B]
    train = grid.extend(i, X[idx0], resident=True)
    both = grid.extend(i, np.vstack([X[idx0], X2]), resident=True)
    i0, i1 = np.arange(m, dtype=np.int32), m + np.arange(NEW, dtype=np.int32)
    ref = both.test_pgbinary_batch(i0, i1, K, ts, Y, SIGMA, 0.0, col=col, seeds=seeds, N_sample=NS, output_pi=True, return_state=True,
                                   return_argmax=True)
    pred, state = make(grid, i, train, i0, K, Y, B, return_state=True)
    assert pred.dims == {"d": d, "s": s, "r": 0, "K": K, "groups": 1, "q": B, "kind": "pg", "ldp": 16}
    np.testing.assert_array_equal(state["omega"], ref["omega"])
    np.testing.assert_array_equal(state["f"], ref["f"])
    got = pred.predict(X2, latent=True)
    compare(got, ref, f"nystrom new rows {shape} a2={A2S[i]} m={m} B={B}", dup)
    # the training rows themselves, served as rows
    ref0 = both.test_pgbinary_batch(i0, i0, K, ts, Y, SIGMA, 0.0, col=col, seeds=seeds, N_sample=NS, output_pi=True, return_argmax=True)
    compare(pred.predict(X[idx0]), ref0, f"nystrom training rows {shape} a2={A2S[i]} m={m} B={B}", dup)
    host = pred.to_host()
    assert (host["P"][:, B:] == 0.0).all() and (host["cg"] == 0.0).all()
    np.testing.assert_array_equal(pred.apply(X2, var=False)["mean"], got["f"])
    with pytest.raises(api.FlgpError, match="predictor_apply: a Polya-Gamma handle has no variance"):
        pred.apply(X2)
    for mp in (1, 2):
        other = make(grid, i, train, i0, K, Y, B, max_parallel=mp)
        np.testing.assert_array_equal(other.to_host()["P"], host["P"])
        other.free()
    train.free(); both.free(); pred.free()


@pytest.mark.parametrize("shape", ["s130", "s200"])
def test_bits_do_not_depend_on_the_call(shape):
    import torch
    n, d, s, K = SHAPES[shape]
    X, U, X2 = cloud(shape)
    grid = grid_of(shape)
    B, m, i = 9, 60, 0
    idx0, Y = problem(shape, m)
    train = grid.extend(i, X[idx0], resident=True)
    pred = make(grid, i, train, np.arange(m, dtype=np.int32), K, Y, B)
    X3 = np.asfortranarray(np.random.default_rng(n + 7).normal(size=(513, d)))
    L = _lib.lib()
    keys = ("f", "pi", "y", "label")
    want = pred.predict(X3, latent=True)
    L.flgp_set_tuning(b"model_extend_block", 256)
    try:
        small = pred.predict(X3, latent=True)
        n_new, ldx, ld = 513, 516, {"f": 518, "pi": 515, "y": 514}
        dX = torch.full((d, ldx), float("nan"), dtype=torch.float64, device=DEV)
        dX[:, :n_new] = torch.from_numpy(np.ascontiguousarray(X3.T)).to(DEV)
        buf = {k: torch.full((B + 1, ld[k]), float("nan"), dtype=torch.float64, device=DEV) for k in ld}
        lab = torch.full((n_new + 3,), float("nan"), dtype=torch.float64, device=DEV)
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(L.flgp_dev_predictor_pg_apply(st, pred._h, dX.data_ptr(), n_new, ldx, buf["f"].data_ptr(), ld["f"],
                                                 buf["pi"].data_ptr(), ld["pi"], buf["y"].data_ptr(), ld["y"], lab.data_ptr()))
        # without the latent the block's f lives in the call's own workspace
        pi2 = torch.full((B + 1, ld["pi"]), float("nan"), dtype=torch.float64, device=DEV)
        _lib.check(L.flgp_dev_predictor_pg_apply(st, pred._h, dX.data_ptr(), n_new, ldx, None, 0, pi2.data_ptr(), ld["pi"], None, 0, None))
        torch.cuda.synchronize()
    finally:
        L.flgp_set_tuning(b"model_extend_block", 1 << 20)
    for k in keys:
        np.testing.assert_array_equal(small[k], want[k], err_msg=k)
    for k in ld:
        a = buf[k].cpu().numpy()
        np.testing.assert_array_equal(a[:B, :n_new].T, want[k], err_msg=k)
        assert np.isnan(a[B]).all() and np.isnan(a[:, n_new:]).all()
    a = lab.cpu().numpy()
    np.testing.assert_array_equal(a[:n_new], want["label"]); assert np.isnan(a[n_new:]).all()
    a = pi2.cpu().numpy()
    np.testing.assert_array_equal(a[:B, :n_new].T, want["pi"]); assert np.isnan(a[B]).all() and np.isnan(a[:, n_new:]).all()
    for r in (0, 255, 256, 300, 512):
        one = pred.predict(X3[r:r + 1], latent=True)
        for k in keys:
            np.testing.assert_array_equal(one[k][0], want[k][r], err_msg=f"{k} row {r}")
    for knob in (0, 1):
        try:
            L.flgp_set_tuning(b"nystrom_dot_gemm", knob)
            other = pred.predict(X3, latent=True)
        finally:
            L.flgp_set_tuning(b"nystrom_dot_gemm", -1)
        for k in keys:
            np.testing.assert_array_equal(other[k], want[k], err_msg=f"{k} nystrom_dot_gemm={knob}")
    np.testing.assert_array_equal(pred.predict(X3)["pi"], want["pi"])
    train.free(); pred.free()


def test_refusals_that_need_a_live_grid():
    shape = "s130"
    n, d, s, K = SHAPES[shape]
    X, U, X2 = cloud(shape)
    grid = grid_of(shape)
    m = 60
    idx0, Y = problem(shape, m)
    i0 = np.arange(m, dtype=np.int32)
    train1 = grid.extend(1, X[idx0], resident=True)
    with pytest.raises(api.FlgpError, match="predictor_nystrom_pg: the pair's values are not those of bandwidth 0"):
        make(grid, 0, train1, i0, K, Y, 3)
    # the bandwidth index comes before the chains' refusals, those before the handle kind's check
    import ctypes
    ts, col, seeds, _ = CHAINS[3]
    sd = np.array(seeds, dtype=np.uint64)
    out = ctypes.c_void_p(1)
    L = _lib.lib()

    def create(i, n_sample, K_):
        return L.flgp_predictor_nystrom_pg_create(grid._h, i, train1._h, K_, i0.ctypes.data, m, Y.ctypes.data, 2, col.ctypes.data,
                                                  ts.ctypes.data, sd.ctypes.data, 3, SIGMA, n_sample, 0, None, None, ctypes.byref(out))
    assert create(2, 0, K) == -1 and L.flgp_last_error().decode() == "predictor_nystrom_pg: bandwidth 2 outside 0..1"
    assert out.value is None
    assert create(0, 0, K) == -1 and L.flgp_last_error().decode() == "predictor_nystrom_pg: N_sample=0 must be at least 1"
    assert create(0, NS, K + 1) == -1 and L.flgp_last_error().decode() == f"predictor_nystrom_pg: need 1 <= K <= {K} (K={K + 1})"
    good = make(grid, 1, train1, i0, K, Y, 3)
    bad = np.array(X2[:40], order="F"); bad[3, 2] = np.inf
    before = good.predict(X2[:40])
    with pytest.raises(api.FlgpError, match="points"):
        good.predict(bad)
    np.testing.assert_array_equal(good.predict(X2[:40])["pi"], before["pi"])
    train1.free(); good.free()
