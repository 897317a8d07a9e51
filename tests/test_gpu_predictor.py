"""GPU (-m gpu): the fitted predictor's handle (include/flgp_hip.h) on the fits of
tests/test_gpu_spectrum_model.py ("A": n 3000, d 3, s 200, r 5, K 20; "As": K = s = 200; "wide": d 70), made once per module.

* fit rows, regression: Predictor.regression(..).apply(X[rows]) against ResidentEigenPair.regression_posterior on the fit's
  pair (the model returns fit rows bit for bit, so no extension is in the reference), to atol_mean / atol_var of
  tests/regression_posterior_cases.py; the measured |d| is printed next to the bound.
* new rows: 300 rows of another draw of the mixture, against model.extend(resident, head) + regression_posterior.
* logit: B = 3 problems against logit_posterior_batch, np_logit_posterior.tolerances and the Newton tol of
  tests/logit_posterior_cases.py; the iteration counts are the batch entry's for m > K; P does not depend on max_parallel.
* bits: 513 rows at model_extend_block = 256, at the default block, one at a time and through flgp_dev_predictor_apply;
  two creates give the same P; P is the restatement's (tests/np_predictor.py) to 1e-12 max|P|.
* the refusals that need live handles."""
import ctypes
import functools

import numpy as np
import pytest

import np_logit_posterior as nlp
import np_predictor as npp
import regression_posterior_cases as rc
from conftest import make_case
from flgp_amd import _lib, api, synth
from logit_posterior_cases import TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = {"A": (3000, 3, 200, 5, 20), "As": (3000, 3, 200, 5, 200), "wide": (600, 70, 64, 5, 10)}
EPSILON = {"A": 0.7, "As": 0.7, "wide": 6.0}
T, NOISE, SIGMA = 2.0, 0.1, 1e-3


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()


@functools.lru_cache(maxsize=None)
def case(shape):
    n, d, s, r, K = SHAPES[shape]
    X, U0, U = make_case(n, d, s, r, seed=n + d)
    for a in (X, U0, U):
        a.setflags(write=False)
    return X, U0, U


@functools.lru_cache(maxsize=None)
def fitted(shape, kernel="lae"):
    """(model, pair, the pair on the host): one fit per configuration, shared and left unchanged"""
    n, d, s, r, K = SHAPES[shape]
    X, U0, U = case(shape)
    model, pair = api.heat_kernel_spectrum_model(X, X[:0], s, r, K, models={"kernel": kernel, "gl": "cluster-normalized", "root": True},
                                                 epsilon=EPSILON[shape], U=U)
    host = pair.to_host()
    host.values.setflags(write=False); host.vectors.setflags(write=False)
    return model, pair, host


def training(shape, m, q, seed):
    n = SHAPES[shape][0]
    X = case(shape)[0]
    rng = np.random.default_rng(seed)
    idx0 = rng.permutation(n)[:m].astype(np.int32)
    Y = np.asfortranarray(np.sin(2.0 * X[idx0, :1] + np.arange(q)[None, :]) + 0.1 * rng.normal(size=(m, q)))
    nz = rng.uniform(0.01, 0.5, m); nz[0] = NOISE
    return idx0, Y, nz


def check_regression(got, ref, host, rows, K, m, c, label):
    """atol_mean / atol_var of the regression posterior's tests; prints |d| next to the bound and returns the two ratios"""
    prior = ((host.vectors[rows, :K] ** 2) * np.exp(-T * (1.0 - host.values[:K]))).sum(1).max()
    bm = rc.atol_mean(ref["posterior"]["mean"])
    bv = rc.atol_var(dict(var=ref["posterior"]["cov"], prior=prior, m=m, c=c))
    dm = np.abs(got["mean"] - ref["posterior"]["mean"]).max()
    dv = np.abs(got["var"][:, 0] - ref["posterior"]["cov"]).max()
    print(f"{label}: mean |d| {dm:.3e} bound {bm:.3e} ratio {dm / bm:.3e}; var |d| {dv:.3e} bound {bv:.3e} ratio {dv / bv:.3e}")
    assert np.abs(ref["posterior"]["mean"]).max() > 0.0
    assert dm <= bm and dv <= bv
    assert (got["var"] >= c).all()
    return dm / bm, dv / bv


# ---------------------------------------------------------------------------------------------- 1. fit rows, regression
FIT_CASES = [("A", 20, 60, 1, "same"), ("A", 20, 60, 3, "same"), ("A", 20, 60, 1, "different"), ("A", 20, 60, 3, "different"),
             ("A", 13, 60, 1, "same"), ("A", 20, 12, 1, "same"), ("As", 200, 260, 1, "same"), ("wide", 10, 60, 3, "different")]


@pytest.mark.parametrize("shape,K,m,q,noisepar", FIT_CASES)
def test_fit_rows_regression(shape, K, m, q, noisepar):
    n = SHAPES[shape][0]
    X = case(shape)[0]
    model, pair, host = fitted(shape)
    idx0, Y, nz = training(shape, m, q, seed=K + m + q)
    rows = np.random.default_rng(5).permutation(n)[:257].astype(np.int32)
    pars = (T, NOISE) if noisepar == "same" else np.r_[T, nz]
    ref = pair.regression_posterior(Y, idx0, rows, K, pars, SIGMA, noisepar=noisepar, train=False)
    pred = api.Predictor.regression(model, pair, Y, idx0, K, pars, SIGMA, noisepar=noisepar)
    assert pred.dims == {"d": SHAPES[shape][1], "s": SHAPES[shape][2], "r": SHAPES[shape][3], "K": K, "groups": 1, "q": q,
                         "kind": "regression", "ldp": (K + q + 15) // 16 * 16}
    got = pred.apply(X[rows])
    check_regression(got, ref, host, rows, K, m, NOISE + SIGMA, f"fit rows {shape} K={K} m={m} q={q} {noisepar}")
    np.testing.assert_array_equal(pred.to_host()["cg"], [NOISE + SIGMA])
    pred.free(); pred.free()
    with pytest.raises(ValueError, match="freed"):
        pred.apply(X[rows])


# ------------------------------------------------------------------------------------------------------- 2. new rows
@pytest.mark.parametrize("kernel", ["lae", "se"])
@pytest.mark.parametrize("shape", ["A", "wide"])
def test_new_rows_regression(shape, kernel):
    n, d, s, r, K = SHAPES[shape]
    model, pair, host = fitted(shape, kernel)
    m, q = 60, 1
    idx0, Y, nz = training(shape, m, q, seed=11)
    X2 = synth.gaussian_mixture(300, d, components=5, seed=n + d + 1000)               # another draw: none of the fit rows
    both = model.extend(X2, resident=True, head=pair, head_rows=idx0)
    i0, i1 = np.arange(m, dtype=np.int32), m + np.arange(300, dtype=np.int32)
    ref = both.regression_posterior(Y, i0, i1, K, (T, NOISE), SIGMA, train=False)
    pred = api.Predictor.regression(model, pair, Y, idx0, K, (T, NOISE), SIGMA)
    got = pred.apply(X2)
    ext = both.to_host()
    check_regression(got, ref, ext, i1, K, m, NOISE + SIGMA, f"new rows {shape} {kernel}")
    both.free(); pred.free()


# ------------------------------------------------------------------------------------------------------------ 3. logit
def logit_problem(shape, m, seed=21):
    X = case(shape)[0]
    idx0 = np.random.default_rng(seed).permutation(SHAPES[shape][0])[:m].astype(np.int32)
    Y = np.asfortranarray(np.stack([(X[idx0, 0] > np.median(X[idx0, 0])).astype(float),
                                    (X[idx0, 1] > np.median(X[idx0, 1])).astype(float)], axis=1))
    return idx0, Y, np.array([0, 1, 1], dtype=np.int32), np.array([1.5, 1.5, 4.0])    # two columns, one of them at two t


@pytest.mark.parametrize("sig", [(0.0, 1e-3), (0.05, 0.0)])
@pytest.mark.parametrize("m", [60, 12])
def test_logit_against_the_batch_entry(m, sig):
    shape = "A"
    n, d, s, r, K = SHAPES[shape]
    X = case(shape)[0]
    model, pair, host = fitted(shape)
    idx0, Y, col, ts = logit_problem(shape, m)
    rows = np.random.default_rng(6).permutation(n)[:257].astype(np.int32)
    ref, its = pair.logit_posterior_batch(idx0, rows, K, ts, Y, col=col, sigma11=sig[0], sigma22=sig[1], tol=TOL, return_iters=True)
    pred = api.Predictor.logit(model, pair, idx0, K, ts, Y, col=col, sigma11=sig[0], sigma22=sig[1], tol=TOL)
    assert (pred.groups, pred.q, pred.kind, pred.ldp) == (3, 1, "logit", (3 * (K + 1) + 15) // 16 * 16)
    got = pred.apply(X[rows])
    if m > K:
        np.testing.assert_array_equal(pred.iters, its)
    for b in range(3):
        C22 = ((host.vectors[rows, :K] ** 2) * nlp.lam_of(host.values, K, ts[b])).sum(1) + sig[1]
        am, av = nlp.tolerances(ref["mean"][:, b], ref["cov"][:, b], C22, m)
        dm = np.abs(got["mean"][:, b] - ref["mean"][:, b]).max(); dv = np.abs(got["var"][:, b] - ref["cov"][:, b]).max()
        print(f"logit m={m} sig={sig} problem {b}: mean |d| {dm:.3e} bound {am:.3e}; var |d| {dv:.3e} bound {av:.3e}")
        assert np.abs(ref["mean"][:, b]).max() > 0.0
        assert dm <= am and dv <= av
    assert (got["var"] >= sig[1]).all()
    np.testing.assert_array_equal(pred.to_host()["cg"], [sig[1]] * 3)
    P = pred.to_host()["P"]
    for mp in (1, 2):
        other = api.Predictor.logit(model, pair, idx0, K, ts, Y, col=col, sigma11=sig[0], sigma22=sig[1], tol=TOL, max_parallel=mp)
        np.testing.assert_array_equal(other.to_host()["P"], P)
        np.testing.assert_array_equal(other.iters, pred.iters)
        other.free()
    pred.free()


# ------------------------------------------------------------------------------------------------------------- 4. bits
def test_apply_bits_do_not_depend_on_the_call():
    import torch
    shape = "A"
    n, d, s, r, K = SHAPES[shape]
    X = case(shape)[0]
    model, pair, host = fitted(shape)
    q = 3
    idx0, Y, nz = training(shape, 60, q, seed=33)
    pred = api.Predictor.regression(model, pair, Y, idx0, K, (T, NOISE), SIGMA)
    X2 = np.asfortranarray(synth.gaussian_mixture(513, d, components=5, seed=99))
    L = _lib.lib()
    want = pred.apply(X2)
    L.flgp_set_tuning(b"model_extend_block", 256)
    try:
        small = pred.apply(X2)
        # the device-pointer entry on padded buffers
        n_new, ldx, ldm, ldv = 513, 516, 518, 515
        dX = torch.full((d, ldx), float("nan"), dtype=torch.float64, device=DEV)
        dX[:, :n_new] = torch.from_numpy(np.ascontiguousarray(X2.T)).to(DEV)
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
    for i in (0, 255, 256, 300, 512):
        one = pred.apply(X2[i:i + 1])
        np.testing.assert_array_equal(one["mean"][0], want["mean"][i]); np.testing.assert_array_equal(one["var"][0], want["var"][i])
    no_var = pred.apply(X2, var=False)
    assert no_var["var"] is None
    np.testing.assert_array_equal(no_var["mean"], want["mean"])
    # two creates, and the restatement of P from the model on the host
    again = api.Predictor.regression(model, pair, Y, idx0, K, (T, NOISE), SIGMA)
    P = pred.to_host()["P"]
    np.testing.assert_array_equal(again.to_host()["P"], P)
    assert (P[:, K + q:] == 0.0).all()                                   # the padding columns
    h = model.to_host()
    V1 = host.vectors[idx0, :K]
    ls = np.sqrt(np.exp(-T * (1.0 - host.values[:K])))
    c = NOISE + SIGMA
    Q = (ls[:, None] * (V1.T @ V1)) * ls[None, :] + c * np.eye(K)
    LQ = np.linalg.cholesky(Q)
    G = np.linalg.solve(LQ, np.eye(K)) * (np.sqrt(c) * ls)[None, :]
    U = ls[:, None] * np.linalg.solve(Q, ls[:, None] * (V1.T @ Y))
    Pn = npp.fold(h["V"], h["eig"], n, G, U)
    dP = np.abs(P[:, :K + q] - Pn).max()
    print(f"P against the restatement: |d| {dP:.3e}, 1e-12 max|P| = {1e-12 * np.abs(Pn).max():.3e}")
    assert dP <= 1e-12 * np.abs(Pn).max()
    again.free(); pred.free()


# ------------------------------------------------------------------------------------------------- 5. live refusals
def test_refusals_that_need_live_handles():
    shape = "A"
    n, d, s, r, K = SHAPES[shape]
    X = case(shape)[0]
    model, pair, host = fitted(shape)
    idx0, Y, nz = training(shape, 60, 1, seed=44)
    # a pair from another fit: the same shape, other values
    other_model, other_pair, _ = fitted(shape, "se")
    with pytest.raises(api.FlgpError, match="predictor_regression: the pair's values are not the model's"):
        api.Predictor.regression(model, other_pair, Y, idx0, K, (T, NOISE), SIGMA)
    with pytest.raises(api.FlgpError, match="predictor_logit: the pair's values are not the model's"):
        api.Predictor.logit(model, other_pair, idx0, K, [1.5], (Y[:, 0] > 0).astype(float))
    # a pair of another K
    narrow = api.ResidentEigenPair.from_host(api.EigenPair(host.values[:13].copy(), np.asfortranarray(host.vectors[:, :13])))
    with pytest.raises(api.FlgpError, match="predictor_regression: the pair has K = 13, the model K = 20"):
        api.Predictor.regression(model, narrow, Y, idx0, 13, (T, NOISE), SIGMA)
    narrow.free()
    with pytest.raises(api.FlgpError, match="predictor_regression: idx0"):
        api.Predictor.regression(model, pair, Y, np.r_[idx0[:-1], n], K, (T, NOISE), SIGMA)
    out = ctypes.c_void_p(1)
    i0 = np.ascontiguousarray(idx0); nzv = np.array([NOISE])
    rc_ = _lib.lib().flgp_predictor_regression_create(model._h, other_pair._h, K, i0.ctypes.data, 60, Y.ctypes.data, 1, T,
                                                      nzv.ctypes.data, 1, SIGMA, ctypes.byref(out))
    assert rc_ == -1 and out.value is None
    # a NaN in X is the input check's refusal, and the handle stays usable
    pred = api.Predictor.regression(model, pair, Y, idx0, K, (T, NOISE), SIGMA)
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
