"""GPU: the Polya-Gamma Gibbs prediction (flgp_amd/csrc/pg.hip).  The sampler's law against the PG(b, c)
moments and Laplace transform; the chains of all three routes against a numpy restatement fed with the same random
numbers (tests/np_pg.py); the law of one f-step and the stationary mean against independent estimates; the multiclass
entry against the binary one; and an end-to-end run at BASELINE configs[2]'s size.  Fixed seeds throughout; every
statistical bound is at least 5 standard errors."""
import os
import sys

import numpy as np
import pytest

from flgp_amd import api, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_pg  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()


def synthetic_pair(n, K, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
    V = np.asfortranarray(scale * rng.standard_normal((n, K)))
    return api.EigenPair(values, V), api.ResidentEigenPair.from_host(api.EigenPair(values, V))


def hk(ep, K, t, i0, i1):
    l, _ = np_pg.weights(ep.values, K, t)
    return (ep.vectors[i0, :K] * l) @ ep.vectors[i1, :K].T


# ---- the sampler --------------------------------------------------------------------------------------------------------
def _log_cosh(x):
    x = np.abs(x)
    return x + np.log1p(np.exp(-2.0 * x)) - np.log(2.0)


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("c", [0.0, 1e-8, 0.5, 2.0, 10.0, 40.0, -3.0, 300.0])
def test_sampler_law(b, c):
    N = 1 << 20
    x = api.pgdraw(b, np.full(N, c), seed=20261015 + b)
    assert np.isfinite(x).all() and (x > 0).all()
    a = abs(c)
    mean = b / 4.0 if a == 0 else b * np.tanh(a / 2) / (2 * a)
    var = b / 24.0 if a < 1e-3 else b * (np.sinh(a) - a) / (4 * a ** 3 * np.cosh(a / 2) ** 2)
    xm = x.mean()
    assert abs(xm - mean) <= 5 * np.sqrt(var / N), (xm, mean)
    d = x - xm
    m4 = (d ** 4).mean()
    xv = (d ** 2).mean()
    assert abs(xv - var) <= 5 * np.sqrt(max(m4 - var ** 2, 0.0) / N) + 1e-15, (xv, var)
    for s in (0.5, 2.0, 10.0, 50.0):
        e = np.exp(-s * x)
        want = np.exp(b * (_log_cosh(c / 2) - _log_cosh(np.sqrt((c * c / 2 + s) / 2))))
        assert abs(e.mean() - want) <= 5 * e.std() / np.sqrt(N) + 1e-15, (s, e.mean(), want)


def test_sampler_reproduces_numpy_and_seed():
    c = np.array([0.0, 1e-8, 0.5, -2.0, 10.0, 40.0, 300.0, 0.3, 1.1, 0.64, 1.5625, 5.0])
    b = np.array([1, 2, 3, 1, 2, 3, 1, 4, 1, 1, 2, 1], dtype=float)
    x = api.pgdraw(b, c, seed=77)
    np.testing.assert_allclose(x, np_pg.pg_draw(c, 77, 3, b), rtol=1e-12, atol=0)
    assert np.array_equal(x, api.pgdraw(b, c, seed=77))
    assert not np.array_equal(x, api.pgdraw(b, c, seed=78))


# ---- exact restatement of the chains ------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,m", [(40, 24), (40, 40), (16, 48), (8, 64)])     # m <= K: the m x m route; m > K: Woodbury
def test_resident_chain_reproduces_numpy(K, m):
    ep, rp = synthetic_pair(300, 40, seed=K + m, scale=0.5)
    rng = np.random.default_rng(m)
    idx0 = np.sort(rng.choice(300, m, replace=False)); idx1 = np.arange(0, 300, 7)
    Y = (rng.uniform(size=m) < 0.4).astype(float)
    t, sigma, seed, ns = 3.0, 1e-2, 1234 + m, 20
    out = rp.test_pgbinary(idx0, idx1, K, t, Y, sigma, sigma, N_sample=ns, output_pi=True, seed=seed, return_state=True)
    l, ls = np_pg.weights(ep.values, K, t)
    V1 = ep.vectors[idx0, :K]
    omega, f, kappa, C, _ = np_pg.chain(Y, ns, seed, sigma=sigma, V1=V1, l=l, ls=ls)
    np.testing.assert_allclose(out["omega"], omega, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(out["f"], f, rtol=1e-9, atol=1e-9)
    w = np_pg.collapsed_w(omega, kappa, C)
    Cnv = hk(ep, K, t, idx1, idx0) + sigma * (idx1[:, None] == idx0[None, :])
    pi = np_pg.logistic(Cnv @ w)
    np.testing.assert_allclose(out["pi_pred"], pi, rtol=1e-9, atol=1e-9)
    assert np.array_equal(out["Y_pred"], (out["pi_pred"] > 0.5).astype(float))
    rp.free()


@pytest.mark.parametrize("m", [5, 32, 64])
def test_dense_chain_reproduces_numpy(m):
    ep, rp = synthetic_pair(200, 30, seed=m, scale=0.5)
    rp.free()
    rng = np.random.default_rng(m + 1)
    idx0 = np.arange(m); idx1 = np.arange(m, 200)
    C = np.asfortranarray(hk(ep, 30, 2.0, idx0, idx0) + 1e-2 * np.eye(m))
    C = np.asfortranarray(0.5 * (C + C.T))
    Cnv = np.asfortranarray(hk(ep, 30, 2.0, idx1, idx0))
    Y = (rng.uniform(size=m) < 0.5).astype(float)
    pi, y, om, f = api._pg_logit_predict_state(C, Y, Cnv, 20, 99 + m)
    omega, fn, kappa, _, _ = np_pg.chain(Y, 20, 99 + m, C=C)
    np.testing.assert_allclose(om, omega, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(f, fn, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(pi, np_pg.logistic(Cnv @ np_pg.collapsed_w(omega, kappa, C)), rtol=1e-9, atol=1e-9)
    assert np.array_equal(y, (pi > 0.5).astype(float))
    r = api.test_pgbinary_cpp(C, Y, Cnv, N_sample=20, output_pi=True, seed=99 + m)
    assert np.array_equal(r["pi_pred"], pi) and np.array_equal(r["Y_pred"], y)
    assert set(api.test_pgbinary_cpp(C, Y, Cnv, N_sample=2, seed=1)) == {"Y_pred"}


# ---- the collapsed prediction from the returned omega ------------------------------------------------------------------
@pytest.mark.parametrize("K,m", [(60, 50), (20, 120)])
@pytest.mark.parametrize("nv", [0.0, 1.0])
def test_collapsed_prediction_from_omega(K, m, nv):
    ep, rp = synthetic_pair(500, 60, seed=5, scale=0.5)
    rng = np.random.default_rng(6)
    idx0 = rng.choice(500, m, replace=False).astype(np.int32)
    idx1 = np.arange(500, dtype=np.int32)                 # every row, as the binary drivers predict
    Y = (rng.uniform(size=m) < 0.5).astype(float)
    t, sigma = 2.5, 3e-2
    snv = nv * sigma
    out = rp.test_pgbinary(idx0, idx1, K, t, Y, sigma, snv, N_sample=5, output_pi=True, seed=8, return_state=True)
    Cvv = hk(ep, K, t, idx0, idx0) + sigma * np.eye(m)
    Cnv = hk(ep, K, t, idx1, idx0) + snv * (idx1[:, None] == idx0[None, :])
    w = np_pg.collapsed_w(out["omega"], Y - 0.5, Cvv)
    np.testing.assert_allclose(out["pi_pred"], np_pg.logistic(Cnv @ w), rtol=1e-10, atol=1e-10)
    rp.free()


# ---- the law of one f-step and the stationary mean -------------------------------------------------------------------
@pytest.mark.parametrize("K", [8, 4])          # m = 6: the m x m route, then Woodbury
def test_law_of_one_f_step(K):
    ep, rp = synthetic_pair(50, 8, seed=21, scale=0.6)
    idx0 = np.array([3, 9, 14, 22, 31, 40]); idx1 = np.array([0])
    Y = np.array([1.0, 0.0, 1.0, 1.0, 0.0, 0.0])
    t, sigma = 2.0, 0.05
    N = 4000
    fs = np.array([rp.test_pgbinary(idx0, idx1, K, t, Y, sigma, 0.0, N_sample=1, seed=s, return_state=True)["f"]
                   for s in range(N)])
    C = hk(ep, K, t, idx0, idx0) + sigma * np.eye(6)
    S = np.linalg.inv(np.linalg.inv(C) + np.eye(6))
    mu = S @ (Y - 0.5)
    se_mu = np.sqrt(np.diag(S) / N)
    assert (np.abs(fs.mean(0) - mu) <= 5 * se_mu).all(), (fs.mean(0) - mu) / se_mu
    emp = np.cov(fs.T, bias=False)
    se_cov = np.sqrt((np.outer(np.diag(S), np.diag(S)) + S ** 2) / N)
    assert (np.abs(emp - S) <= 5 * se_cov).all(), (emp - S) / se_cov
    rp.free()


def test_stationary_mean_matches_importance_sampling():
    ep, rp = synthetic_pair(50, 8, seed=21, scale=0.6)
    idx0 = np.array([3, 9, 14, 22, 31, 40]); idx1 = np.array([0])
    Y = np.array([1.0, 0.0, 1.0, 1.0, 0.0, 0.0])
    t, sigma, K = 2.0, 0.05, 8
    N = 1500
    fs = np.array([rp.test_pgbinary(idx0, idx1, K, t, Y, sigma, 0.0, N_sample=30, seed=10_000 + s, return_state=True)["f"]
                   for s in range(N)])
    C = hk(ep, K, t, idx0, idx0) + sigma * np.eye(6)
    rng = np.random.default_rng(3)
    prior = rng.standard_normal((1_000_000, 6)) @ np.linalg.cholesky(C).T
    logw = (Y * -np.logaddexp(0, -prior) + (1 - Y) * -np.logaddexp(0, prior)).sum(1)
    w = np.exp(logw - logw.max())
    est = (w[:, None] * prior).sum(0) / w.sum()
    se_is = np.sqrt((w[:, None] ** 2 * (prior - est) ** 2).sum(0)) / w.sum()
    se_g = fs.std(0, ddof=1) / np.sqrt(N)
    assert (np.abs(fs.mean(0) - est) <= 5 * np.sqrt(se_is ** 2 + se_g ** 2)).all(), \
        (fs.mean(0) - est) / np.sqrt(se_is ** 2 + se_g ** 2)
    rp.free()


# ---- multiclass, determinism, errors -------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,m", [(24, 20), (12, 60)])
def test_multiclass_is_the_binary_entry_per_class(K, m):
    ep, rp = synthetic_pair(400, 24, seed=31, scale=0.5)
    rng = np.random.default_rng(32)
    idx0 = rng.choice(400, m, replace=False); idx1 = np.arange(0, 400, 3)
    Y = rng.integers(0, 3, m).astype(float)
    ts = np.array([1.5, 2.5, 4.0]); sigma, seed = 1e-2, 500
    labels, probs = rp.predict_logit_mult_gp_cpp(idx0, idx1, K, ts, Y, sigma, N_sample=15, seed=seed, output_probs=True)
    aug = api.multi_train_split(Y)
    for j in range(3):
        pj = rp.test_pgbinary(idx0, idx1, K, ts[j], aug[:, j], sigma, 0.0, N_sample=15, output_pi=True, seed=seed + j)["pi_pred"]
        assert np.array_equal(probs[:, j], pj), j
    assert np.array_equal(labels, np.argmax(probs, axis=1).astype(float))
    rp.free()


def test_determinism_and_seed():
    ep, rp = synthetic_pair(300, 30, seed=41, scale=0.5)
    idx0 = np.arange(100); idx1 = np.arange(100, 300)
    Y = (np.arange(100) % 3 == 0).astype(float)
    a = rp.test_pgbinary(idx0, idx1, 30, 2.0, Y, 1e-2, 1e-2, N_sample=10, output_pi=True, seed=5, return_state=True)
    b = rp.test_pgbinary(idx0, idx1, 30, 2.0, Y, 1e-2, 1e-2, N_sample=10, output_pi=True, seed=5, return_state=True)
    c = rp.test_pgbinary(idx0, idx1, 30, 2.0, Y, 1e-2, 1e-2, N_sample=10, output_pi=True, seed=6, return_state=True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a["omega"], c["omega"])
    rp.free()


def test_resident_errors():
    ep, rp = synthetic_pair(100, 10, seed=51)
    Y = np.array([0.0, 1.0, 1.0])
    with pytest.raises(api.FlgpError) as e:
        rp.test_pgbinary([0, 1, 2], [5], 11, 1.0, Y, 1e-2, 0.0, seed=1)
    assert e.value.code == -1 and "K" in e.value.message
    with pytest.raises(api.FlgpError) as e:
        rp.test_pgbinary([0, 1, 100], [5], 10, 1.0, Y, 1e-2, 0.0, seed=1)
    assert e.value.code == -1 and "out of range" in e.value.message
    with pytest.raises(api.FlgpError) as e:
        rp.test_pgbinary([0, 1, 2], [-1], 10, 1.0, Y, 1e-2, 0.0, seed=1)
    assert e.value.code == -1 and "out of range" in e.value.message
    with pytest.raises(api.FlgpError) as e:
        rp.predict_logit_mult_gp_cpp([0, 1, 2], [5], 0, [1.0, 1.0], Y, 1e-2, seed=1)
    assert e.value.code == -1
    with pytest.raises(api.FlgpError) as e:
        rp.predict_logit_mult_gp_cpp([0, 1, 2], [500], 5, [1.0, 1.0], Y, 1e-2, seed=1)
    assert e.value.code == -1 and "out of range" in e.value.message
    rp.free()


# ---- end to end at BASELINE configs[2]'s size ---------------------------------------------------------------------------
def test_end_to_end_separable_mixture():
    n, d, s, r, K, m = 1_000_000, 16, 5000, 10, 200, 1000
    seed = 20241022
    X = synth.gaussian_mixture(n, d, components=16, seed=seed)
    comp = np.minimum((synth.uniform(seed, 2, n) * 16).astype(np.int64), 15)
    lab = (comp % 2).astype(float)
    U = synth.anchors_from_rows(X, synth.random_anchor_rows(n, s, seed=seed))
    rp = api.heat_kernel_spectrum_resident(X[:m], X[m:], s, r, K=K, U=U)
    idx0 = np.arange(m); idx1 = np.arange(m, n)
    Y = lab[:m]
    sigma = 1e-3
    ts = [0.5, 1.0, 2.0, 5.0, 10.0, 20.0]
    t = max(ts, key=lambda tt: rp.marginal_log_likelihood_logit_la(K, tt, idx0, Y, sigma=sigma))
    out = rp.test_pgbinary(idx0, idx1, K, t, Y, sigma, sigma, N_sample=100, output_pi=True, seed=2026, return_state=True)
    acc = (out["Y_pred"] == lab[m:]).mean()
    assert acc >= 0.95, (t, acc)
    post = rp.posterior_distribution_classification(idx0, idx1, K, t, Y, sigma, sigma)
    agree = (out["Y_pred"] == (post["mean"] > 0).astype(float)).mean()
    assert agree >= 0.99, (t, agree)
    again = rp.test_pgbinary(idx0, idx1, K, t, Y, sigma, sigma, N_sample=100, output_pi=True, seed=2026, return_state=True)
    for k in out:
        assert np.array_equal(out[k], again[k]), k
    other = rp.test_pgbinary(idx0, idx1, K, t, Y, sigma, sigma, N_sample=100, seed=2027, return_state=True)
    assert not np.array_equal(out["omega"], other["omega"])
    rp.free()
