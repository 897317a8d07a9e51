"""GPU: the regression posterior on the resident pair (flgp_eigenpair_regression_posterior): m <= K is the
three existing entries bit for bit; the weight-space route for m > K against the oracle's reference-form functions under
the project's tolerances (tests/test_gpu_parity.py: 1e-9 max|ref| for the mean, 1e-9 max|ref| + 2e-15 prior m / (noise +
sigma) for the variance) across the 16-row MFMA tile, the q mean rows in / at the end of / across a tile, the row blocks of
the fused kernel, both noise models and three index styles; cov >= noise[0] + sigma exactly; a row's bits against m_new,
position and neighbours, cov's against Y and q; the q = 64 and K = 1024 switches to the GEMM route; the score on the
device; many rows; NaN in Y and the argument checks.

The problems and their references are those of tests/regression_posterior_cases.py: one reference per problem on its 300
new rows, shared by the eight m_new (each a prefix of the 300)."""
import ctypes
import os
import sys

import numpy as np
import pytest

from flgp_amd import _lib, api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regression_posterior_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

MODELS = ["same", "different"]


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()


def resident(values, V):
    return api.ResidentEigenPair.from_host(api.EigenPair(values, V))


@pytest.fixture(scope="module")
def pair():
    values, V = cases.host_pair()
    rp = resident(values, V)
    yield values, V, rp
    rp.free()


def pars_of(t, nz, model):
    return (t, nz[0]) if model == "same" else np.r_[t, nz]


def check(out, p, model, sel, what, train=True):
    """out against the references of problem p (rows `sel` of its new rows)."""
    test, cov = out["Y_pred"]["test"], out["posterior"]["cov"]
    assert out["posterior"]["mean"] is test
    ref = p[model][sel]
    dm = np.abs(test - ref).max(); dc = np.abs(cov - p["var"][sel]).max()
    line = f"{what}: |dtest| {dm:.3e} (atol {cases.atol_mean(p[model]):.3e})  |dcov| {dc:.3e} (atol {cases.atol_var(p):.3e})"
    if train:
        dt = np.abs(out["Y_pred"]["train"] - p["train_" + model]).max()
        line += f"  |dtrain| {dt:.3e} (atol {cases.atol_mean(p['train_' + model]):.3e})"
    print(line)
    assert np.isfinite(test).all() and np.isfinite(cov).all(), what
    assert dm <= cases.atol_mean(p[model]), what
    assert dc <= cases.atol_var(p), what
    assert (cov >= p["c"]).all(), what
    if train:
        assert dt <= cases.atol_mean(p["train_" + model]), what


# ---- 1. m <= K: the three existing entries ------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("m", [40, 17])
def test_dense_route_is_the_existing_entries(pair, m, model):
    _, _, rp = pair
    K, mnew, sigma = 40, 129, 1e-3
    for perm in (False, True):
        rng = np.random.default_rng(m + 100 * perm)
        idx0 = rng.permutation(cases.N)[:m] if perm else np.arange(50, 50 + m)
        idx1 = rng.permutation(cases.N)[:mnew] if perm else np.arange(1000, 1000 + mnew)
        Y = rng.standard_normal((m, 2))
        pars = pars_of(3.0, rng.uniform(0.01, 0.5, m), model)
        new = rp.regression_posterior(Y, idx0, idx1, K, pars, sigma, model)
        assert np.array_equal(new["Y_pred"]["train"], rp.predict_regression_cpp(Y, idx0, idx0, K, pars, sigma, model))
        assert np.array_equal(new["Y_pred"]["test"], rp.predict_regression_cpp(Y, idx0, idx1, K, pars, sigma, model))
        assert np.array_equal(new["posterior"]["cov"], rp.posterior_covariance_regression(idx0, idx1, K, pars[:2], sigma))


# ---- 2. m > K: the weight-space route against the reference form ---------------------------------------------------------
@pytest.mark.parametrize("style", list(cases.STYLES))
@pytest.mark.parametrize("K,m,q", cases.GRID + cases.TILE)
def test_weight_space_route_against_the_reference(pair, K, m, q, style):
    _, _, rp = pair
    p = cases.problem(K, m, q, style)
    for model in MODELS:
        pars = pars_of(p["t"], p["nz"], model)
        full = rp.regression_posterior(p["Y"], p["idx0"], p["idx1"], K, pars, p["sigma"], model)
        check(full, p, model, slice(None), f"K={K} m={m} q={q} {style} {model} m_new=300")
        for mnew in cases.MNEW[:-1]:
            part = rp.regression_posterior(p["Y"], p["idx0"], p["idx1"][:mnew], K, pars, p["sigma"], model, train=False)
            check(part, p, model, slice(0, mnew), f"K={K} m={m} q={q} {style} {model} m_new={mnew}", train=False)
            # a row's bits do not depend on how many rows follow it
            assert part["Y_pred"]["test"].tobytes() == np.asfortranarray(full["Y_pred"]["test"][:mnew]).tobytes(), mnew
            assert part["posterior"]["cov"].tobytes() == full["posterior"]["cov"][:mnew].tobytes(), mnew


# ---- 3. a row's bits are its own; cov's do not depend on Y or q -----------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("K", [65, 129, 200])      # 64-, 32- and 32-row blocks
def test_a_rows_bits_are_its_own(pair, K, model):
    _, _, rp = pair
    rng = np.random.default_rng(K)
    m, row = 2 * K + 37, 1234
    idx0 = rng.permutation(cases.N)[:m]
    Y = rng.standard_normal((m, 3))
    pars = pars_of(2.0, rng.uniform(0.01, 0.5, m), model)
    others = np.setdiff1d(np.arange(cases.N), [row])
    a = np.arange(row, row + 200)
    b = rng.permutation(others)[:129]; b[70] = row
    c = rng.permutation(others)[:17]; c[3] = row; c[11] = row
    got = []
    for idx1, at in ((a, [0]), (b, [70]), (c, [3, 11])):
        out = rp.regression_posterior(Y, idx0, idx1, K, pars, 1e-3, model, train=False)
        again = rp.regression_posterior(Y, idx0, idx1, K, pars, 1e-3, model, train=False)
        assert out["Y_pred"]["test"].tobytes() == again["Y_pred"]["test"].tobytes()
        assert out["posterior"]["cov"].tobytes() == again["posterior"]["cov"].tobytes()
        got += [(out["Y_pred"]["test"][i].tobytes(), out["posterior"]["cov"][i].tobytes()) for i in at]
    assert len(got) == 4 and all(g == got[0] for g in got)
    # the training rows go through the same kernel: row `row` as a training row, predicted in place
    idx0[5] = row
    out = rp.regression_posterior(Y, idx0, np.array([row]), K, pars, 1e-3, model)
    assert out["Y_pred"]["train"][5].tobytes() == out["Y_pred"]["test"][0].tobytes()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("K", [47, 64, 200])       # K + q rows end inside a tile; K a multiple of 16; 32-row blocks
def test_cov_does_not_depend_on_Y_or_q(pair, K, model):
    _, _, rp = pair
    rng = np.random.default_rng(K + 1)
    m = 2 * K + 5
    idx0 = rng.permutation(cases.N)[:m]; idx1 = rng.permutation(cases.N)[:300]
    pars = pars_of(2.0, rng.uniform(0.01, 0.5, m), model)
    one = rp.regression_posterior(rng.standard_normal((m, 1)), idx0, idx1, K, pars, 1e-3, model, train=False)
    many = rp.regression_posterior(rng.standard_normal((m, 17)), idx0, idx1, K, pars, 1e-3, model, train=False)
    assert one["posterior"]["cov"].tobytes() == many["posterior"]["cov"].tobytes()


def test_different_with_equal_variances_is_same(pair):
    _, _, rp = pair
    p = cases.problem(64, 133, 2, "perm_overlap")
    same = rp.regression_posterior(p["Y"], p["idx0"], p["idx1"], 64, (p["t"], 0.2), p["sigma"])
    diff = rp.regression_posterior(p["Y"], p["idx0"], p["idx1"], 64, np.r_[p["t"], np.full(133, 0.2)], p["sigma"], "different")
    for k in ("train", "test"):
        assert np.abs(diff["Y_pred"][k] - same["Y_pred"][k]).max() <= 1e-9 * np.abs(same["Y_pred"][k]).max()
    assert diff["posterior"]["cov"].tobytes() == same["posterior"]["cov"].tobytes()      # the same Q_s, the same launches


# ---- 4. the limits of the fused kernel: q = 64 and K = 1024, the GEMM route beyond ---------------------------------------
def prof_count(name):
    c = ctypes.c_int(); ms = ctypes.c_double(); w = ctypes.c_double()
    _lib.lib().flgp_prof_query(name.encode(), ctypes.addressof(c), ctypes.addressof(ms), ctypes.addressof(w))
    return c.value


@pytest.fixture(scope="module")
def wide_pair():
    values, V = cases.host_pair(1200, 1030, 135)
    rp = resident(values, V)
    yield values, V, rp
    rp.free()


def routed(rp, *args):
    """The call and how many row passes took the fused kernel and the GEMM route."""
    L = _lib.lib()
    L.flgp_prof_reset(); L.flgp_prof_enable(2)
    try:
        out = rp.regression_posterior(*args)
        routes = prof_count("gpr_predict_rows"), prof_count("gpr_predict_rows_wide")
    finally:
        L.flgp_prof_enable(0); L.flgp_prof_reset()
    return out, routes


def wide_problem(values, V, K, m, q, perm, mnew=100):
    n = V.shape[0]
    rng = np.random.default_rng(K + q + perm)
    idx0 = rng.permutation(n)[:m] if perm else np.arange(m)
    idx1 = rng.permutation(n)[:mnew] if perm else np.arange(n - mnew, n)
    Y = np.asfortranarray(rng.standard_normal((m, q)))
    nz = rng.uniform(0.05, 0.5, m); nz[0] = 0.1
    p = dict(K=K, m=m, q=q, t=0.5, sigma=1e-3, idx0=idx0, idx1=idx1, Y=Y, nz=nz)
    p.update(cases.references(values, V, Y, idx0, idx1, K, 0.5, nz, 1e-3))
    return p


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("perm", [False, True], ids=["range", "perm"])
@pytest.mark.parametrize("K,fused", [(1025, False), (1024, True)])
def test_wide_k(wide_pair, K, fused, perm, model):
    values, V, rp = wide_pair
    p = wide_problem(values, V, K, 1100, 2, perm)
    out, routes = routed(rp, p["Y"], p["idx0"], p["idx1"], K, pars_of(p["t"], p["nz"], model), p["sigma"], model)
    assert routes == ((2, 0) if fused else (0, 2))          # the training rows and the new rows
    check(out, p, model, slice(None), f"K={K} {model}")


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("perm", [False, True], ids=["range", "perm"])
def test_q_limit(wide_pair, perm, model):
    values, V, rp = wide_pair
    K = 40
    p = wide_problem(values, V, K, 85, 65, perm)
    pars = pars_of(p["t"], p["nz"], model)
    wide, routes = routed(rp, p["Y"], p["idx0"], p["idx1"], K, pars, p["sigma"], model)
    assert routes == (0, 2)
    check(wide, p, model, slice(None), f"q=65 {model}")
    fused, routes = routed(rp, p["Y"][:, :64], p["idx0"], p["idx1"], K, pars, p["sigma"], model)
    assert routes == (2, 0)
    for k in ("same", "different", "train_same", "train_different"):
        p[k] = p[k][:, :64]
    check(fused, p, model, slice(None), f"q=64 {model}")
    # the two routes agree to rounding, not in bits
    assert np.abs(fused["Y_pred"]["test"] - wide["Y_pred"]["test"][:, :64]).max() <= cases.atol_mean(p[model])
    assert np.abs(fused["posterior"]["cov"] - wide["posterior"]["cov"]).max() <= cases.atol_var(p)


# ---- 5. the score where the result lies --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,m", [(63, 200), (40, 17)])      # the weight-space route and the dense one
@pytest.mark.parametrize("mnew", [1, 300, 4097])
def test_nll_is_the_host_entry_on_the_delivered_arrays(pair, K, m, mnew):
    _, _, rp = pair
    rng = np.random.default_rng(K + mnew)
    idx0 = rng.permutation(cases.N)[:m]; idx1 = rng.integers(0, cases.N, mnew)
    Y = rng.standard_normal(m); target = rng.standard_normal(mnew)
    for model in MODELS:
        pars = pars_of(2.0, rng.uniform(0.01, 0.5, m), model)
        out = rp.regression_posterior(Y, idx0, idx1, K, pars, 1e-3, model, target=target)
        host = api.negative_log_likelihood(out["posterior"]["mean"][:, 0], out["posterior"]["cov"], target, "regression")
        assert np.isfinite(host) and out["nll"] == host
        plain = rp.regression_posterior(Y, idx0, idx1, K, pars, 1e-3, model)
        assert plain["posterior"]["mean"].tobytes() == out["posterior"]["mean"].tobytes() and "nll" not in plain
        only = rp.regression_posterior(Y, idx0, idx1, K, pars, 1e-3, model, target=target, return_posterior=False)
        assert only == {"nll": host}


# ---- 6. many rows ---------------------------------------------------------------------------------------------------------
def test_many_rows():
    n, K, m, t, sigma = 120_000, 80, 1000, 2.0, 1e-3
    values, V = cases.host_pair(n, K, 137)
    rp = resident(values, V)
    rng = np.random.default_rng(138)
    idx0 = rng.permutation(n)[:m]
    Y = rng.standard_normal((m, 2))
    nz = rng.uniform(0.01, 0.5, m); nz[0] = 0.05
    sample = np.sort(rng.permutation(n)[:2000])
    p = dict(cases.references(values, V, Y, idx0, sample, K, t, nz, sigma))
    for model in MODELS:
        out = rp.regression_posterior(Y, idx0, np.arange(n), K, pars_of(t, nz, model), sigma, model)
        assert (out["posterior"]["cov"] >= p["c"]).all()
        sub = {"Y_pred": {"train": out["Y_pred"]["train"], "test": out["Y_pred"]["test"][sample]},
               "posterior": {"mean": None, "cov": out["posterior"]["cov"][sample]}}
        sub["posterior"]["mean"] = sub["Y_pred"]["test"]
        check(sub, p, model, slice(None), f"2000 of {n} rows, {model}")
    rp.free()


# ---- 7. behaviour ---------------------------------------------------------------------------------------------------------
def test_nan_in_Y_comes_back_as_nan_means(pair):
    _, _, rp = pair
    for K, m in ((40, 100), (40, 30)):
        rng = np.random.default_rng(m)
        idx0 = rng.permutation(cases.N)[:m]; idx1 = np.arange(2000, 2050)
        Y = rng.standard_normal((m, 2)); Y[3, 0] = np.nan
        out = rp.regression_posterior(Y, idx0, idx1, K, (2.0, 0.1), 1e-3)          # status OK
        assert np.isnan(out["Y_pred"]["test"][:, 0]).all() and np.isnan(out["Y_pred"]["train"][:, 0]).all()
        assert np.isfinite(out["Y_pred"]["test"][:, 1]).all() and np.isfinite(out["Y_pred"]["train"][:, 1]).all()
        assert np.isfinite(out["posterior"]["cov"]).all() and (out["posterior"]["cov"] >= 0.1 + 1e-3).all()


def _raw(rp, K=20, m=30, mnew=5, q=1, idx0=None, idx1=None, nz=None, n_noise=1, t=1.0, sigma=1e-3):
    idx0 = np.arange(m, dtype=np.int32) if idx0 is None else np.ascontiguousarray(idx0, dtype=np.int32)
    idx1 = np.arange(100, 100 + mnew, dtype=np.int32) if idx1 is None else np.ascontiguousarray(idx1, dtype=np.int32)
    nz = np.full(m, 0.1) if nz is None else np.ascontiguousarray(nz, dtype=np.float64)
    Y = np.zeros((m, q), order="F"); tr = np.zeros((m, q), order="F"); te = np.zeros((mnew, q), order="F"); cv = np.zeros(mnew)
    return _lib.lib().flgp_eigenpair_regression_posterior(rp._h, K, idx0.ctypes.data, m, idx1.ctypes.data, mnew, Y.ctypes.data, q, t,
                                                          nz.ctypes.data, n_noise, sigma, tr.ctypes.data, te.ctypes.data,
                                                          cv.ctypes.data, None, None)


def test_invalid_arguments():
    n = 500
    values, V = cases.host_pair(n, 20, 139)
    rp = resident(values, V)
    L = _lib.lib()
    assert _raw(rp) == 0 and _raw(rp, m=10) == 0 and _raw(rp, n_noise=30) == 0 and _raw(rp, t=-1.0) == 0       # valid
    bad = {
        "K > ep.K": dict(K=21),
        "idx0 out of range": dict(idx0=np.r_[np.arange(29), n]),
        "idx0 negative": dict(idx0=np.r_[-1, np.arange(29)]),
        "idx1 out of range": dict(idx1=np.r_[np.arange(4), n]),
        "idx1 negative": dict(idx1=np.r_[np.arange(4), -1]),
        "noise + sigma = 0": dict(nz=np.full(30, -1e-3)),
        "noise[7] + sigma < 0": dict(nz=np.r_[np.full(7, 0.1), -0.5, np.full(22, 0.1)], n_noise=30),
        "noise nan": dict(nz=np.full(30, np.nan)),
    }
    for name, kw in bad.items():
        assert _raw(rp, **kw) == -1, name
        assert L.flgp_last_error().decode().startswith("regression_posterior:"), (name, L.flgp_last_error())
    with pytest.raises(api.FlgpError) as e:
        rp.regression_posterior(np.zeros(30), np.arange(30), np.array([0, n]), 20, (1.0, 0.1), 1e-3)
    assert e.value.code == -1 and "out of range" in e.value.message
    out = rp.regression_posterior(np.zeros(30), np.arange(30), np.arange(100, 105), 20, (1.0, 0.1), 1e-3)    # still works
    assert (out["Y_pred"]["test"] == 0).all() and (out["posterior"]["cov"] >= 0.1 + 1e-3).all()
    rp.free()
