"""GPU: the regression training objectives on the resident pair (include/flgp_hip.h) against the numpy
restatement of negative_{marginal_likelihood,log_posterior}{,_diff_noise}_regression_cpp (src/train.cpp:333-555) in
tests/np_regression_objective.py."""
import os
import sys

import numpy as np
import pytest

from flgp_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_regression_objective as R  # noqa: E402

pytestmark = pytest.mark.gpu

N, KP = 3000, 48          # pair size; every case uses K = KP, so m <= 48 is the direct branch
KW = 1200                 # the wide pair of the block- and stride-edge cases


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()


@pytest.fixture(scope="module")
def pair():
    rng = np.random.default_rng(5)
    values, V = R.synthetic_pair(N, KP, rng)
    rp = api.ResidentEigenPair.from_host(api.EigenPair(values, V))
    yield values, V, rp
    rp.free()


@pytest.fixture(scope="module")
def wide_pair():
    """K up to 1200 > 1024: the direct branch reaches m > 1024 (multi-block tri_inverse, chol_logdet and rg_assemble
    loops past their 1024-thread stride) and K > 1024 in rg_assemble's k-loops; Woodbury runs at small K and m = 2500."""
    rng = np.random.default_rng(1200)
    values, V = R.synthetic_pair(N, KW, rng)
    rp = api.ResidentEigenPair.from_host(api.EigenPair(values, V))
    yield values, V, rp
    rp.free()


def rows(kind, m, rng):
    return np.arange(100, 100 + m) if kind == "range" else rng.choice(N, m, replace=False)


def xs(noise, m, rng, t=2.0, lo=0.05, hi=0.4):
    return np.r_[t, 0.2] if noise == "same" else np.r_[t, rng.uniform(lo, hi, m)]


def close(dev, ref):
    (v, g), (vr, gr) = dev, ref
    assert abs(v - vr) <= 1e-9 * abs(vr), (v, vr)
    assert np.abs(g - gr).max() <= 1e-8 * max(1.0, np.abs(gr).max()), np.abs(g - gr).max()


@pytest.mark.parametrize("kind", ["range", "scattered"])
@pytest.mark.parametrize("q", [1, 3])
@pytest.mark.parametrize("m", [30, KP, KP + 1, 150], ids=["direct", "m=K", "m=K+1", "woodbury"])
@pytest.mark.parametrize("approach", ["marginal", "posterior"])
@pytest.mark.parametrize("noise", ["same", "different"])
def test_against_restatement(pair, noise, approach, m, q, kind):
    values, V, rp = pair
    rng = np.random.default_rng(m * 7 + q)
    idx = rows(kind, m, rng)
    Y = rng.standard_normal((m, q))
    x = xs(noise, m, rng)
    dev = rp.regression_objective(x, KP, idx, Y, sigma=1e-5, noise=noise, approach=approach)
    close(dev, R.objective(values, V, KP, idx, Y, x, 1e-5, noise, approach))


# Each edge of the dense layer once under "same" and once under "different", the approaches and q in {1, 5, 70} spread
# over them: direct (K = 1200 >= m) at m across the 64-wide blocks and the 1024 stride; Woodbury at K across one block
# with m = K + 1 and m = 2500 (rg_assemble's per-row loop of "different" wraps twice).
EDGE_CASES = [
    # noise, approach, m, K, q
    ("same", "marginal", 1, KW, 1), ("different", "posterior", 1, KW, 5),
    ("same", "posterior", 63, KW, 70), ("different", "marginal", 63, KW, 1),
    ("same", "marginal", 64, KW, 5), ("different", "posterior", 64, KW, 70),
    ("same", "posterior", 65, KW, 1), ("different", "marginal", 65, KW, 5),
    ("same", "marginal", 129, KW, 70), ("different", "posterior", 129, KW, 1),
    ("same", "posterior", 1025, KW, 5), ("different", "marginal", 1025, KW, 70),
    ("same", "marginal", 1100, KW, 1), ("different", "posterior", 1100, KW, 5),
    ("same", "marginal", 2, 1, 1), ("different", "posterior", 2500, 1, 5),
    ("same", "posterior", 2500, 63, 70), ("different", "marginal", 64, 63, 1),
    ("same", "marginal", 65, 64, 5), ("different", "posterior", 2500, 64, 70),
    ("same", "posterior", 2500, 65, 1), ("different", "marginal", 66, 65, 5),
    ("same", "marginal", 130, 129, 70), ("different", "posterior", 2500, 129, 1),
]


@pytest.mark.parametrize("noise,approach,m,K,q", EDGE_CASES,
                         ids=[f"{n}-{a}-m{m}-K{k}-q{q}" for n, a, m, k, q in EDGE_CASES])
def test_block_and_stride_edges(wide_pair, noise, approach, m, K, q):
    values, V, rp = wide_pair
    rng = np.random.default_rng(m * 131 + K * 7 + q)
    idx = rows("scattered", m, rng)
    Y = rng.standard_normal((m, q))
    x = xs(noise, m, rng)
    dev = rp.regression_objective(x, K, idx, Y, sigma=1e-5, noise=noise, approach=approach)
    assert dev[1].shape == ((m + 1) if noise == "different" else 2,)
    close(dev, R.objective(values, V, K, idx, Y, x, 1e-5, noise, approach))


@pytest.mark.parametrize("m,scale", [(30, 10.0), (150, 1.0)], ids=["direct", "woodbury"])
def test_same_noise_clipping(pair, m, scale):
    """grad_1 of "same" is clipped at 10 in both branches when the noise is small, and not when it is large."""
    values, V, rp = pair
    rng = np.random.default_rng(m)
    idx = rows("scattered", m, rng)
    Y = scale * rng.standard_normal((m, 2))
    for x1, clipped in ((0.2, True), (20.0, False)):
        x = np.r_[2.0, x1]
        ref = R.objective(values, V, KP, idx, Y, x, 1e-5, "same", "marginal")
        assert (abs(ref[1][1]) == 10.0) == clipped
        close(rp.regression_objective(x, KP, idx, Y, noise="same", approach="marginal"), ref)


def test_different_noise_clipping(pair):
    """grad_1..m of "different" is clipped at 1 in the Woodbury branch: a mix of clipped and free entries."""
    values, V, rp = pair
    rng = np.random.default_rng(3)
    m = 150
    idx = rows("scattered", m, rng)
    Y = 3.0 * rng.standard_normal((m, 1))
    x = np.r_[2.0, np.where(np.arange(m) % 2 == 0, 0.05, 2.0)]
    for approach in ("marginal", "posterior"):
        ref = R.objective(values, V, KP, idx, Y, x, 1e-5, "different", approach)
        if approach == "marginal":
            free = np.abs(ref[1][1:]) < 1.0
            assert free.any() and not free.all()
        close(rp.regression_objective(x, KP, idx, Y, noise="different", approach=approach), ref)


@pytest.mark.parametrize("noise", ["same", "different"])
@pytest.mark.parametrize("m", [30, 150], ids=["direct", "woodbury"])
def test_gradient_is_the_derivative_of_the_value(pair, noise, m):
    values, V, rp = pair
    rng = np.random.default_rng(m + 1)
    idx = rows("scattered", m, rng)
    Y = 0.3 * rng.standard_normal((m, 2))
    x = np.r_[2.0, 20.0] if noise == "same" else xs(noise, m, rng, lo=0.6, hi=1.0)
    v, g = rp.regression_objective(x, KP, idx, Y, noise=noise, approach="posterior")
    ref = R.objective(values, V, KP, idx, Y, x, 1e-5, noise, "posterior")
    _, gu = R.objective(values, V, KP, idx, Y, x, 1e-5, noise, "posterior", clip=False)
    assert np.array_equal(ref[1], gu), "the case must be unclipped"
    f = lambda z: rp.regression_objective(z, KP, idx, Y, noise=noise, approach="posterior", grad=False)  # noqa: E731
    fd = R.central_diff(f, x, 1e-5)
    assert np.abs(g - fd).max() <= 1e-5 * max(1.0, np.abs(g).max())


@pytest.mark.parametrize("m", [30, 150], ids=["direct", "woodbury"])
def test_equal_noises_match_same(pair, m):
    """"different" with every noise equal is "same" -- up to the reference's 1e-9 regularisers in the Woodbury value:
    log(L_ii + 1e-9) of Q there, of Q / c and log(z_i + 1e-9) here; the gap is the restatement's own."""
    values, V, rp = pair
    rng = np.random.default_rng(m + 2)
    idx = rows("scattered", m, rng)
    Y = rng.standard_normal((m, 2))
    xd = np.r_[2.0, np.full(m, 0.3)]
    vs, gs = rp.regression_objective([2.0, 0.3], KP, idx, Y, noise="same", approach="marginal")
    vd, gd = rp.regression_objective(xd, KP, idx, Y, noise="different", approach="marginal")
    gap = R.nmll(values, V, KP, idx, Y, xd, 1e-5, "different")[0] - R.nmll(values, V, KP, idx, Y, [2.0, 0.3], 1e-5)[0]
    assert (gap == 0.0) == (m <= KP)
    assert abs((vd - vs) - gap) <= 1e-10 * abs(vs)
    assert abs(gd[0] - gs[0]) <= 1e-8 * max(1.0, abs(gs[0]))


@pytest.mark.parametrize("noise", ["same", "different"])
@pytest.mark.parametrize("m", [30, 150], ids=["direct", "woodbury"])
def test_value_only_and_repeatable(pair, noise, m):
    values, V, rp = pair
    rng = np.random.default_rng(m + 3)
    idx = rows("scattered", m, rng)
    Y = rng.standard_normal((m, 3))
    x = xs(noise, m, rng)
    v1, g1 = rp.regression_objective(x, KP, idx, Y, noise=noise)
    v2, g2 = rp.regression_objective(x, KP, idx, Y, noise=noise)
    assert v1 == v2 and np.array_equal(g1, g2)
    assert rp.regression_objective(x, KP, idx, Y, noise=noise, grad=False) == v1


def test_singular_system_is_reported_or_finite(pair):
    """A repeated row with noise + sigma = 1e-300 makes C singular in fp64: FLGP_ERR_NOCONV or finite numbers, the same
    outcome twice, never a NaN."""
    _, _, rp = pair
    idx = np.array([5, 9, 5, 17, 40])
    Y = np.arange(5.0)
    outcomes = []
    for _ in range(2):
        try:
            v, g = rp.regression_objective([2.0, 0.0], KP, idx, Y, sigma=1e-300, approach="marginal")
            assert np.isfinite(v) and np.isfinite(g).all()
            outcomes.append((v, tuple(g)))
        except api.FlgpError as e:
            assert e.code == -5
            outcomes.append(e.code)
    assert outcomes[0] == outcomes[1]


def test_refusals(pair):
    _, _, rp = pair
    idx = np.arange(10)
    Y = np.zeros(10)
    with pytest.raises(api.FlgpError) as e:
        rp.regression_objective([2.0, 0.2], KP + 1, idx, Y)
    assert e.value.code == -1
    with pytest.raises(api.FlgpError) as e:
        rp.regression_objective([2.0, 0.2, 0.3], KP, idx, Y)                 # nx = 3 for "same"
    assert e.value.code == -1
    with pytest.raises(api.FlgpError) as e:
        rp.regression_objective([2.0, 0.2], KP, idx, Y, noise="different")   # nx = 2 for m = 10 "different"
    assert e.value.code == -1
    with pytest.raises(api.FlgpError) as e:
        rp.regression_objective([2.0, 0.2], KP, np.r_[idx[:-1], N], Y)
    assert e.value.code == -1 and "out of range" in e.value.message
    with pytest.raises(api.FlgpError) as e:
        rp.regression_objective([0.0, 0.2], KP, idx, Y)                      # t <= 0 under "posterior"
    assert e.value.code == -1
    with pytest.raises(api.FlgpError) as e:
        rp.regression_objective([2.0, np.nan], KP, idx, Y)
    assert e.value.code == -1
    with pytest.raises(api.FlgpError) as e:
        rp.regression_objective([2.0, -1.0], KP, idx, Y)                     # noise + sigma <= 0
    assert e.value.code == -1
    with pytest.raises(api.FlgpError) as e:
        rp.regression_objective([2.0, 0.2], KP, idx, Y, noise="equal")
    assert e.value.code == -3 and e.value.message == "The noise setting is illegal!"
    with pytest.raises(ValueError):
        rp.regression_objective([2.0, 0.2], KP, idx, np.zeros(9))


@pytest.mark.parametrize("n,K,noises", [(1_000_000, 200, ("same", "different")), (100_000, 2000, ("same", "different"))],
                         ids=["woodbury_n1e6_K200", "direct_n1e5_K2000"])
def test_full_size(n, K, noises):
    rng = np.random.default_rng(n + K)
    values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
    V = np.asfortranarray(rng.standard_normal((n, K)))
    rp = api.ResidentEigenPair.from_host(api.EigenPair(values, V))
    try:
        m = 1000
        idx = rng.choice(n, m, replace=False)
        Y = rng.standard_normal((m, 1))
        for noise in noises:
            x = xs(noise, m, rng, t=3.0)
            close(rp.regression_objective(x, K, idx, Y, noise=noise), R.objective(values, V, K, idx, Y, x, 1e-5, noise))
    finally:
        rp.free()
