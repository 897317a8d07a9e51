"""GPU: the predictive negative log likelihood (flgp_amd/csrc/nll.hip) against a numpy restatement fed with
the same random numbers (tests/np_nll.py), at the wave, workgroup and slab edges of the kernel and of flgp_dev_mean; the
multinomial route against the binary one, bit for bit; the reference's edge arithmetic; 64-bit counters; and the law of
the value against independent numpy replicates, the link to the reference's rnorm.  Fixed seeds throughout.

Bounds on the restatement: 1e-12 absolute on like, 1e-10 absolute on the value.  Box-Muller's absolute error is about
1e-14 (cos of an argument rounded at 6.28, times a radius <= 8.6); the logistic function's slope is <= 1/4, so like moves
by less than sqrt(cov) 3e-15 <= 1.2e-14 at these inputs, and the log's slope is <= 100: two orders of margin for the
device's exp / log against libm's."""
import os
import sys

import numpy as np
import pytest

from flgp_amd import _lib, api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_nll  # noqa: E402

pytestmark = pytest.mark.gpu

LIKE_TOL, VALUE_TOL = 1e-12, 1e-10
SLABS = 3 * 4096 + 5


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()


# ---- 1. binary against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_samples", [(n, 100) for n in (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, SLABS)]
                         + [(257, ns) for ns in (1, 2, 99, 101)])
def test_binary_reproduces_numpy(n, n_samples):
    mean, cov, y = np_nll.inputs(n, seed=1000 * n_samples + n)
    seed = 20261018 + n
    value, like = api.negative_log_likelihood(mean, cov, y, "binary", n_samples=n_samples, seed=seed, return_like=True)
    ref_value, ref_like = np_nll.nll_classification(mean, cov, y, n_samples, seed)
    print("binary", n, n_samples, np.abs(like - ref_like).max(), abs(value - ref_value))
    assert like.shape == (n,)
    assert np.abs(like - ref_like).max() <= LIKE_TOL
    assert abs(value - ref_value) <= VALUE_TOL
    assert api.nll_classification(mean, cov, y, n_samples=n_samples, seed=seed) == value


# ---- 2. multinomial ----------------------------------------------------------------------------------------------------
def dev_class_value(mean, cov, y, n_samples, seed, stream0):
    """one class through the device-pointer entry, on the stream stream0: (value, like)"""
    import torch
    L = _lib.lib()
    n = mean.size
    dm, dc, dy = (torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda") for a in (mean, cov, y))
    like = torch.zeros(n, dtype=torch.float64, device="cuda"); out = torch.zeros(1, dtype=torch.float64, device="cuda")
    work = torch.zeros(L.flgp_dev_nll_workspace(n, 1) // 8, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    _lib.check(L.flgp_dev_nll_classification(torch.cuda.current_stream().cuda_stream, dm.data_ptr(), dc.data_ptr(), dy.data_ptr(),
                                             n, 1, 0, n_samples, seed, stream0, like.data_ptr(), out.data_ptr(), work.data_ptr()))
    torch.cuda.synchronize()
    return float(out.cpu()[0]), like.cpu().numpy()


@pytest.mark.parametrize("J", [2, 3, 10])
@pytest.mark.parametrize("n", [65, 4097])
def test_multinomial(n, J):
    mean, cov, labels = np_nll.inputs(n, seed=50 * n + J, J=J)
    seed = 77 + J
    value, like = api.negative_log_likelihood(mean, cov, labels, "multinomial", seed=seed, return_like=True)
    ref_value, ref_like = np_nll.nll_multinomial(mean, cov, labels, 100, seed)
    print("multinomial", n, J, np.abs(like - ref_like).max(), abs(value - ref_value))
    assert like.shape == (n, J)
    assert np.abs(like - ref_like).max() <= LIKE_TOL
    assert abs(value - ref_value) <= VALUE_TOL
    # column 0 is the binary call on multi_train_split's first column, bit for bit: its like array and its value, the
    # latter through the device-pointer entry, which also gives the other classes' values (stream0 = j); the J values
    # are added in class order from 0.0
    aug = api.multi_train_split(labels)
    v0, like0 = api.negative_log_likelihood(mean[:, 0], cov[:, 0], aug[:, 0], "binary", seed=seed, return_like=True)
    assert np.array_equal(like0, like[:, 0])
    total = 0.0
    for j in range(J):
        vj, like_j = dev_class_value(mean[:, j], cov[:, j], aug[:, j], 100, seed, j)
        assert np.array_equal(like_j, like[:, j])
        if j == 0:
            assert vj == v0
        total += vj
    assert total == value
    assert api.negative_log_likelihood(mean, cov, labels, "multinomial", seed=seed + 1) != value


# ---- 3. regression -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, 4097, SLABS])
def test_regression(n):
    rng = np.random.default_rng(n)
    mean = rng.standard_normal(n); y = mean + 0.5 * rng.standard_normal(n); cov = rng.uniform(0.05, 2.0, n)
    value, terms = api.negative_log_likelihood(mean, cov, y, "regression", return_like=True)
    ref_value, ref_terms = np_nll.nll_regression(mean, cov, y)
    print("regression", n, abs(value - ref_value) / abs(ref_value), np.abs(terms - ref_terms).max())
    assert abs(value - ref_value) <= 1e-12 * abs(ref_value)
    np.testing.assert_allclose(terms, ref_terms, rtol=1e-13, atol=1e-13)
    with_pi = (ref_terms.mean() + np.log(2 * np.pi)) / 2
    assert abs(value - with_pi) > 1e-9                      # the reference's truncated constant is part of the contract
    assert api.negative_log_likelihood(mean, cov, y, "regression", n_samples=0, seed=3) == value      # both ignored


# ---- 4. edge values ----------------------------------------------------------------------------------------------------
def test_zero_variance_rows():
    mean, cov, y = np_nll.inputs(300, seed=41)
    cov[::3] = 0.0
    y[:] = 1.0
    _, like = api.nll_classification(mean, cov, y, seed=4, return_like=True)
    assert np.abs(like[::3] - np_nll.logistic(mean[::3])).max() <= 1e-15
    y[:] = 0.0
    _, like = api.nll_classification(mean, cov, y, seed=4, return_like=True)
    assert np.abs(like[::3] - (1.0 - np_nll.logistic(mean[::3]))).max() <= 1e-15


@pytest.mark.parametrize("mean,y,like_want,term_want", [
    (800.0, 1.0, 1.0, -np.log(1.01)), (800.0, 0.0, 0.0, -np.log(1e-2)),
    (-800.0, 1.0, 0.0, -np.log(1e-2)), (-800.0, 0.0, 1.0, -np.log(1.01)),      # exp(800) overflows: pi = 0
])
def test_saturated_means(mean, y, like_want, term_want):
    value, like = api.nll_classification([mean], [4.0], [y], seed=5, return_like=True)     # n = 1: the value is the row term
    assert np.isfinite(value)
    assert abs(like[0] - like_want) <= 1e-15
    assert abs(value - term_want) <= 1e-15


def test_negative_variance_gives_nan_and_touches_no_other_row():
    mean, cov, y = np_nll.inputs(4097, seed=43)
    cov0 = cov.copy(); cov0[1234] = 0.0
    cov[1234] = -1.0
    value, like = api.nll_classification(mean, cov, y, seed=6, return_like=True)
    value0, like0 = api.nll_classification(mean, cov0, y, seed=6, return_like=True)
    assert np.isnan(value) and np.isnan(like[1234]) and np.isfinite(value0)
    keep = np.arange(4097) != 1234
    assert np.array_equal(like[keep], like0[keep])


def test_non_binary_target_is_used_linearly():
    mean, cov, y = np_nll.inputs(257, seed=44)
    y[::2] = 0.3
    value, like = api.nll_classification(mean, cov, y, seed=7, return_like=True)
    ref_value, ref_like = np_nll.nll_classification(mean, cov, y, 100, 7)
    assert np.abs(like - ref_like).max() <= LIKE_TOL and abs(value - ref_value) <= VALUE_TOL
    _, like1 = api.nll_classification(mean, cov, np.ones(257), seed=7, return_like=True)      # like = 0.3 E pi + 0.7 E (1 - pi)
    assert np.abs(like[::2] - (0.3 * like1[::2] + 0.7 * (1.0 - like1[::2]))).max() <= 1e-14


# ---- 5. determinism ----------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    mean, cov, labels = np_nll.inputs(SLABS, seed=45, J=3)
    a = api.negative_log_likelihood(mean, cov, labels, "multinomial", seed=8, return_like=True)
    b = api.negative_log_likelihood(mean, cov, labels, "multinomial", seed=8, return_like=True)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


# ---- 6. 64-bit counters ------------------------------------------------------------------------------------------------
def test_counters_pass_2_31_and_2_32():
    """2 i n_samples passes 2^31 between rows 26 843 and 26 844 and 2^32 between 53 687 and 53 688"""
    n, n_samples, seed = 70_001, 40_000, 9
    rows = np.array([0, 26_843, 26_844, 53_687, 53_688, 70_000])
    assert 2 * 26_843 * n_samples < 2 ** 31 <= 2 * 26_844 * n_samples and 2 * 53_687 * n_samples < 2 ** 32 <= 2 * 53_688 * n_samples
    mean, cov, y = np_nll.inputs(n, seed=46)
    _, like = api.nll_classification(mean, cov, y, n_samples=n_samples, seed=seed, return_like=True)
    ref = np_nll.like_rows(mean, cov, y, n_samples, seed, 0, rows=rows)
    print("counters", np.abs(like[rows] - ref).max())
    assert np.abs(like[rows] - ref).max() <= 1e-12


# ---- 7. law ------------------------------------------------------------------------------------------------------------
def test_law_against_independent_replicates():
    """The device value for seeds 1 .. 8 within 5 standard deviations of the mean of 200 replicates of the numpy route on
    numpy's own normals, the sd that of the replicates.  With the restatement in place of the device the eight z-scores
    lie between -0.67 and +0.35.  A kernel that reuses one sample vector for every row passes this test and fails the
    restatement tests, one with a wrong law the reverse: that is why both are there."""
    n, n_samples = 4097, 100
    mean, cov, y = np_nll.inputs(n, seed=47)
    reps = np.array([np_nll.value_from_like(np_nll.like_from_normals(
        mean, cov, y, np.random.default_rng([1, i]).standard_normal((n, n_samples)))) for i in range(200)])
    mu, sd = reps.mean(), reps.std(ddof=1)
    for seed in range(1, 9):
        v = api.nll_classification(mean, cov, y, n_samples=n_samples, seed=seed)
        print("law", seed, (v - mu) / sd)
        assert abs(v - mu) <= 5 * sd, (seed, v, mu, sd)


# ---- 8. end to end -----------------------------------------------------------------------------------------------------
def test_posterior_then_nll_multinomial():
    n, K, m, J = 3000, 40, 200, 3
    rng = np.random.default_rng(48)
    values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
    V = np.asfortranarray(rng.standard_normal((n, K)))
    rp = api.ResidentEigenPair.from_host(api.EigenPair(values, V))
    idx0 = rng.permutation(n)[:m]; idx1 = np.setdiff1d(np.arange(n), idx0)
    Y = rng.integers(0, J, m).astype(np.float64)
    post = rp.posterior_distribution_multiclassification(idx0, idx1, K, [1.0, 2.5, 4.0], Y, 1e-3)
    rp.free()
    labels = rng.integers(0, J, idx1.size).astype(np.float64)
    labels[:J] = np.arange(J)
    value, like = api.negative_log_likelihood(post["mean"], post["cov"], labels, "multinomial", seed=10, return_like=True)
    ref_value, ref_like = np_nll.nll_multinomial(post["mean"], post["cov"], labels, 100, 10)
    assert np.isfinite(value)
    assert np.abs(like - ref_like).max() <= LIKE_TOL
    assert abs(value - ref_value) <= VALUE_TOL
