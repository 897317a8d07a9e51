"""GPU (-m gpu): the Nystrom predictor's handle (include/flgp_hip.h) on the clouds and bandwidths of
tests/test_gpu_nystrom_grid.py -- (n, d, s, K) = (900, 9, 130, 8), (1500, 40, 200, 12), (3000, 64, 257, 5), (600, 70, 96, 4),
a2 in (0.7, 1.0) -- one grid and one training pair per shape, made once per module.  Every comparison is against the route
that exists without the handle: grid.extend(i, fit rows stacked on the new rows, resident=True) + the posterior entry.

* regression: the fit rows and 300 new rows of another draw, to atol_mean / atol_var of tests/regression_posterior_cases.py;
  q 1 and 3, noise "same" and "different", m = 60 > K and m = 10 <= K = 12; |d| is printed next to the bound.
* logit, B = 3: against logit_posterior_batch at np_logit_posterior.tolerances; the iteration counts are the batch entry's for
  m > K; P does not depend on max_parallel.
* bits: 513 rows at model_extend_block = 256, one at a time, through flgp_dev_predictor_apply, at nystrom_dot_gemm 0 and 1,
  without the variance; two creates give the same P; P is the restatement's (tests/np_nystrom_predictor.py) to 1e-12 max|P|.
* the refusals that need live handles, in the order the header states (the device refusal needs a second device and is the
  model-backed handle's check, word for word: it is not provoked here)."""
import ctypes
import functools

import numpy as np
import pytest

import np_logit_posterior as nlp
import np_nystrom_predictor as nnp
import regression_posterior_cases as rc
from flgp_amd import _lib, api
from logit_posterior_cases import TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = {"s130": (900, 9, 130, 8), "s200": (1500, 40, 200, 12), "s257": (3000, 64, 257, 5), "s96": (600, 70, 96, 4)}
A2S = (0.7, 1.0)
T, NOISE, SIGMA = 2.0, 0.1, 1e-3
NEW = 300


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
def fitted(shape):
    """(grid, per bandwidth: the resident pair of the fit rows, the resident pair of the fit rows stacked on the new rows and
    its host copy): shared and left unchanged"""
    n, d, s, K = SHAPES[shape]
    X, U, X2 = cloud(shape)
    grid = api.nystrom_spectrum_grid(U, A2S, K, max_parallel=len(A2S))
    pairs, both, hosts = [], [], []
    for i in range(len(A2S)):
        pairs.append(grid.extend(i, X, resident=True))
        both.append(grid.extend(i, np.vstack([X, X2]), resident=True))
        h = both[i].to_host()
        h.values.setflags(write=False); h.vectors.setflags(write=False)
        hosts.append(h)
    return grid, pairs, both, hosts


def training(shape, m, q, seed):
    n = SHAPES[shape][0]
    X = cloud(shape)[0]
    rng = np.random.default_rng(seed)
    idx0 = rng.permutation(n)[:m].astype(np.int32)
    Y = np.asfortranarray(np.sin(2.0 * X[idx0, :1] + np.arange(q)[None, :]) + 0.1 * rng.normal(size=(m, q)))
    nz = rng.uniform(0.01, 0.5, m); nz[0] = NOISE
    return idx0, Y, nz


def check_regression(got, ref, host, rows, K, m, c, label):
    """atol_mean / atol_var of the regression posterior's tests, unchanged; prints |d| next to the bound"""
    prior = ((host.vectors[rows, :K] ** 2) * np.exp(-T * (1.0 - host.values[:K]))).sum(1).max()
    bm = rc.atol_mean(ref["posterior"]["mean"])
    bv = rc.atol_var(dict(var=ref["posterior"]["cov"], prior=prior, m=m, c=c))
    dm = np.abs(got["mean"] - ref["posterior"]["mean"]).max()
    dv = np.abs(got["var"][:, 0] - ref["posterior"]["cov"]).max()
    print(f"{label}: mean |d| {dm:.3e} bound {bm:.3e} ratio {dm / bm:.3e}; var |d| {dv:.3e} bound {bv:.3e} ratio {dv / bv:.3e}")
    assert np.abs(ref["posterior"]["mean"]).max() > 0.0
    assert dm <= bm and dv <= bv
    assert (got["var"] >= c).all()


# ------------------------------------------------------------------------------------------------------ 1. regression
REGRESSION = [("s130", 0, 8, 60, 1, "same"), ("s130", 1, 8, 60, 3, "different"), ("s130", 0, 5, 60, 3, "same"),
              ("s200", 0, 12, 60, 3, "same"), ("s200", 1, 12, 60, 1, "different"), ("s200", 1, 12, 10, 1, "same"),
              ("s200", 0, 12, 10, 3, "different"), ("s257", 0, 5, 60, 1, "same"), ("s96", 0, 4, 60, 3, "different")]


@pytest.mark.parametrize("shape,i,K,m,q,noisepar", REGRESSION)
def test_regression_against_the_extension_route(shape, i, K, m, q, noisepar):
    n, d, s, Kg = SHAPES[shape]
    X, U, X2 = cloud(shape)
    grid, pairs, both, hosts = fitted(shape)
    idx0, Y, nz = training(shape, m, q, seed=K + m + q)
    pars = (T, NOISE) if noisepar == "same" else np.r_[T, nz]
    pred = api.Predictor.nystrom_regression(grid, i, pairs[i], Y, idx0, K, pars, SIGMA, noisepar=noisepar)
    assert pred.dims == {"d": d, "s": s, "r": 0, "K": K, "groups": 1, "q": q, "kind": "regression", "ldp": (K + q + 15) // 16 * 16}
    np.testing.assert_array_equal(pred.to_host()["cg"], [NOISE + SIGMA])
    fit_rows = np.random.default_rng(5).permutation(n)[:257].astype(np.int32)
    new_rows = (n + np.arange(NEW)).astype(np.int32)
    for rows, Xr, label in ((fit_rows, X[fit_rows], "fit rows"), (new_rows, X2, "new rows")):
        ref = both[i].regression_posterior(Y, idx0, rows, K, pars, SIGMA, noisepar=noisepar, train=False)
        got = pred.apply(Xr)
        check_regression(got, ref, hosts[i], rows, K, m, NOISE + SIGMA, f"{label} {shape} a2={A2S[i]} K={K} m={m} q={q} {noisepar}")
    pred.free(); pred.free()
    with pytest.raises(ValueError, match="freed"):
        pred.apply(X2)


# ------------------------------------------------------------------------------------------------------------ 2. logit
def logit_problem(shape, m, seed=21):
    X = cloud(shape)[0]
    idx0 = np.random.default_rng(seed).permutation(SHAPES[shape][0])[:m].astype(np.int32)
    Y = np.asfortranarray(np.stack([(X[idx0, 0] > np.median(X[idx0, 0])).astype(float),
                                    (X[idx0, 1] > np.median(X[idx0, 1])).astype(float)], axis=1))
    return idx0, Y, np.array([0, 1, 1], dtype=np.int32), np.array([1.5, 1.5, 4.0])    # two columns, one of them at two t


@pytest.mark.parametrize("sig", [(0.0, 1e-3), (0.05, 0.0)])
@pytest.mark.parametrize("shape,i,m", [("s130", 0, 60), ("s200", 1, 60), ("s200", 0, 10)])
def test_logit_against_the_batch_entry(shape, i, m, sig):
    n, d, s, K = SHAPES[shape]
    X, U, X2 = cloud(shape)
    grid, pairs, both, hosts = fitted(shape)
    host = hosts[i]
    idx0, Y, col, ts = logit_problem(shape, m)
    rows = (n + np.arange(NEW)).astype(np.int32)
    ref, its = both[i].logit_posterior_batch(idx0, rows, K, ts, Y, col=col, sigma11=sig[0], sigma22=sig[1], tol=TOL, return_iters=True)
    pred = api.Predictor.nystrom_logit(grid, i, pairs[i], idx0, K, ts, Y, col=col, sigma11=sig[0], sigma22=sig[1], tol=TOL)
    assert (pred.groups, pred.q, pred.r, pred.kind, pred.ldp) == (3, 1, 0, "logit", (3 * (K + 1) + 15) // 16 * 16)
    got = pred.apply(X2)
    if m > K:
        np.testing.assert_array_equal(pred.iters, its)
    for b in range(3):
        C22 = ((host.vectors[rows, :K] ** 2) * nlp.lam_of(host.values, K, ts[b])).sum(1) + sig[1]
        am, av = nlp.tolerances(ref["mean"][:, b], ref["cov"][:, b], C22, m)
        dm = np.abs(got["mean"][:, b] - ref["mean"][:, b]).max(); dv = np.abs(got["var"][:, b] - ref["cov"][:, b]).max()
        print(f"logit {shape} m={m} sig={sig} problem {b}: mean |d| {dm:.3e} bound {am:.3e} ratio {dm / am:.3e}; "
              f"var |d| {dv:.3e} bound {av:.3e} ratio {dv / av:.3e}")
        assert np.abs(ref["mean"][:, b]).max() > 0.0
        assert dm <= am and dv <= av
    assert (got["var"] >= sig[1]).all()
    np.testing.assert_array_equal(pred.to_host()["cg"], [sig[1]] * 3)
    P = pred.to_host()["P"]
    for mp in (1, 2):
        other = api.Predictor.nystrom_logit(grid, i, pairs[i], idx0, K, ts, Y, col=col, sigma11=sig[0], sigma22=sig[1], tol=TOL,
                                            max_parallel=mp)
        np.testing.assert_array_equal(other.to_host()["P"], P)
        np.testing.assert_array_equal(other.iters, pred.iters)
        other.free()
    pred.free()


# ------------------------------------------------------------------------------------------------------------- 3. bits
def test_apply_bits_do_not_depend_on_the_call():
    import torch
    shape, i, q = "s130", 0, 3
    n, d, s, K = SHAPES[shape]
    X, U, _ = cloud(shape)
    grid, pairs, both, hosts = fitted(shape)
    idx0, Y, nz = training(shape, 60, q, seed=33)
    pred = api.Predictor.nystrom_regression(grid, i, pairs[i], Y, idx0, K, (T, NOISE), SIGMA)
    X3 = np.asfortranarray(np.random.default_rng(99).normal(size=(513, d)))
    L = _lib.lib()
    want = pred.apply(X3)
    L.flgp_set_tuning(b"model_extend_block", 256)
    try:
        small = pred.apply(X3)
        n_new, ldx, ldm, ldv = 513, 516, 518, 515                          # the device-pointer entry on padded buffers
        dX = torch.full((d, ldx), float("nan"), dtype=torch.float64, device=DEV)
        dX[:, :n_new] = torch.from_numpy(np.ascontiguousarray(X3.T)).to(DEV)
        dm = torch.full((q + 1, ldm), float("nan"), dtype=torch.float64, device=DEV)
        dv = torch.full((2, ldv), float("nan"), dtype=torch.float64, device=DEV)
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(L.flgp_dev_predictor_apply(st, pred._h, dX.data_ptr(), n_new, ldx, dm.data_ptr(), ldm, dv.data_ptr(), ldv))
        torch.cuda.synchronize()
    finally:
        L.flgp_set_tuning(b"model_extend_block", 1 << 20)
    for key in ("mean", "var"):
        np.testing.assert_array_equal(small[key], want[key])
    dm = dm.cpu().numpy(); dv = dv.cpu().numpy()
    np.testing.assert_array_equal(dm[:q, :n_new].T, want["mean"]); np.testing.assert_array_equal(dv[0, :n_new], want["var"][:, 0])
    assert np.isnan(dm[q]).all() and np.isnan(dm[:, n_new:]).all() and np.isnan(dv[1]).all() and np.isnan(dv[:, n_new:]).all()
    for r in (0, 255, 256, 300, 512):
        one = pred.apply(X3[r:r + 1])
        np.testing.assert_array_equal(one["mean"][0], want["mean"][r]); np.testing.assert_array_equal(one["var"][0], want["var"][r])
    for knob in (0, 1):
        try:
            L.flgp_set_tuning(b"nystrom_dot_gemm", knob)
            other = pred.apply(X3)
        finally:
            L.flgp_set_tuning(b"nystrom_dot_gemm", -1)
        for key in ("mean", "var"):
            np.testing.assert_array_equal(other[key], want[key], err_msg=f"nystrom_dot_gemm={knob}")
    no_var = pred.apply(X3, var=False)
    assert no_var["var"] is None
    np.testing.assert_array_equal(no_var["mean"], want["mean"])
    # two creates, and the restatement of P from what the grid gives out: V' from the extension of the anchors themselves,
    # ext(U) = A V' with A = diag(f) Z_UU (cond(A) is about 1e4 at this bandwidth: the solve is refined with long-double
    # residuals, so that what is left is the rounding of ext(U) itself)
    again = api.Predictor.nystrom_regression(grid, i, pairs[i], Y, idx0, K, (T, NOISE), SIGMA)
    P = pred.to_host()["P"]
    np.testing.assert_array_equal(again.to_host()["P"], P)
    assert (P[:, K + q:] == 0.0).all()                                   # the padding columns
    inv_c = 1.0 / (A2S[i] * grid.distances_mean)
    Zuu = nnp.similarity(U, U, inv_c)
    w = 1.0 / (Zuu.sum(1) + 1e-9)
    A = nnp.row_factor(Zuu, w)[:, None] * Zuu
    E = grid.extend(i, U).vectors
    print(f"cond(A) = {np.linalg.cond(A):.3e}")
    Vp = np.linalg.solve(A, E)
    for _ in range(3):
        resid = (E.astype(np.longdouble) - A.astype(np.longdouble) @ Vp.astype(np.longdouble)).astype(np.float64)
        Vp = Vp + np.linalg.solve(A, resid)
    host = pairs[i].to_host()
    V1 = host.vectors[idx0, :K]
    ls = np.sqrt(np.exp(-T * (1.0 - host.values[:K])))
    c = NOISE + SIGMA
    Q = (ls[:, None] * (V1.T @ V1)) * ls[None, :] + c * np.eye(K)
    LQ = np.linalg.cholesky(Q)
    G = np.linalg.solve(LQ, np.eye(K)) * (np.sqrt(c) * ls)[None, :]
    Uo = ls[:, None] * np.linalg.solve(Q, ls[:, None] * (V1.T @ Y))
    Pn = nnp.fold(Vp, G, Uo)
    dP = np.abs(P[:, :K + q] - Pn).max()
    print(f"P against the restatement: |d| {dP:.3e}, 1e-12 max|P| = {1e-12 * np.abs(Pn).max():.3e}")
    assert dP <= 1e-12 * np.abs(Pn).max()
    again.free(); pred.free()


# ------------------------------------------------------------------------------------------------- 4. live refusals
def test_refusals_that_need_live_handles():
    shape = "s130"
    n, d, s, K = SHAPES[shape]
    X, U, X2 = cloud(shape)
    grid, pairs, both, hosts = fitted(shape)
    idx0, Y, nz = training(shape, 60, 1, seed=44)
    L = _lib.lib()
    i0 = np.ascontiguousarray(idx0); nzv = np.array([NOISE]); ts = np.array([1.5]); yb = np.asfortranarray((Y > 0).astype(float))

    def raw_regression(i=0, pair=None, K_=K, m=60):
        out = ctypes.c_void_p(1)
        rc_ = L.flgp_predictor_nystrom_regression_create(grid._h, i, (pair or pairs[0])._h, K_, i0.ctypes.data, m, Y.ctypes.data, 1, T,
                                                         nzv.ctypes.data, 1, SIGMA, ctypes.byref(out))
        return rc_, out.value, L.flgp_last_error().decode()

    def raw_logit(i=0, pair=None, K_=K):
        out = ctypes.c_void_p(1)
        rc_ = L.flgp_predictor_nystrom_logit_create(grid._h, i, (pair or pairs[0])._h, K_, i0.ctypes.data, 60, yb.ctypes.data, 1, None,
                                                    ts.ctypes.data, 1, 0.0, 1e-3, 1e-5, 10, 0, None, ctypes.byref(out))
        return rc_, out.value, L.flgp_last_error().decode()

    narrow = api.ResidentEigenPair.from_host(api.EigenPair(hosts[0].values[:5].copy(), np.asfortranarray(hosts[0].vectors[:n, :5])))
    # the bandwidth index comes before the mirrored entry's checks (K = 0 is one of them) ...
    for i in (-1, len(A2S)):
        assert raw_regression(i=i, K_=0) == (-1, None, f"predictor_nystrom_regression: bandwidth {i} outside 0..{len(A2S) - 1}")
        assert raw_logit(i=i, K_=0) == (-1, None, f"predictor_nystrom_logit: bandwidth {i} outside 0..{len(A2S) - 1}")
    # ... those before the pair's K against the grid's ...
    rc_, h, msg = raw_regression(pair=narrow, m=0)
    assert (rc_, h) == (-1, None) and msg.startswith("predictor_nystrom_regression: bad shape")
    rc_, h, msg = raw_logit(pair=narrow, K_=0)
    assert (rc_, h) == (-1, None) and msg.startswith("predictor_nystrom_logit: bad shape")
    with pytest.raises(api.FlgpError, match="predictor_nystrom_regression: idx0"):
        api.Predictor.nystrom_regression(grid, 0, pairs[0], Y, np.r_[idx0[:-1], n], K, (T, NOISE), SIGMA)
    # ... and K before the values: the narrow pair's values are not the grid's first 5 either way
    assert raw_regression(pair=narrow, K_=5) == (-1, None, "predictor_nystrom_regression: the pair has K = 5, the grid K = 8")
    assert raw_logit(pair=narrow, K_=5) == (-1, None, "predictor_nystrom_logit: the pair has K = 5, the grid K = 8")
    narrow.free()
    # a pair from another bandwidth: the first device work
    with pytest.raises(api.FlgpError, match="predictor_nystrom_regression: the pair's values are not those of bandwidth 0"):
        api.Predictor.nystrom_regression(grid, 0, pairs[1], Y, idx0, K, (T, NOISE), SIGMA)
    with pytest.raises(api.FlgpError, match="predictor_nystrom_logit: the pair's values are not those of bandwidth 1"):
        api.Predictor.nystrom_logit(grid, 1, pairs[0], idx0, K, ts, yb)
    assert raw_regression(i=1)[:2] == (-1, None)
    # a NaN in X is the input check's refusal, and the handle stays usable
    pred = api.Predictor.nystrom_regression(grid, 0, pairs[0], Y, idx0, K, (T, NOISE), SIGMA)
    good = pred.apply(X[:70])
    bad = np.array(X[:70], order="F"); bad[17, 1] = np.nan
    with pytest.raises(api.FlgpError, match="points"):
        pred.apply(bad)
    after = pred.apply(X[:70])
    for key in ("mean", "var"):
        np.testing.assert_array_equal(after[key], good[key])
    with pytest.raises(ValueError, match="columns"):
        pred.apply(np.zeros((4, d + 1)))
    pred.free()
    with pytest.raises(ValueError, match="freed"):
        pred.apply(X[:70])
    with pytest.raises(ValueError, match="freed"):
        pred.to_host()
