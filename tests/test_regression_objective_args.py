"""CPU: the regression training objective's entry (include/flgp_hip.h) checks its strings and pointers before
any device work, and the numpy restatement the GPU tests compare against is pinned here by central differences."""
import ctypes
import os
import sys

import numpy as np
import pytest

from flgp_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_regression_objective as R  # noqa: E402


def _call(ep, noise, approach, m=3, nx=2, K=2):
    idx = np.arange(m, dtype=np.int32)
    Y = np.zeros(m)
    x = np.full(nx, 0.5)
    v = ctypes.c_double()
    g = np.zeros(nx)
    return _lib.lib().flgp_eigenpair_regression_objective(ep, K, idx.ctypes.data, m, Y.ctypes.data, 1, 1e-5, noise, approach,
                                                          None, x.ctypes.data, nx, ctypes.byref(v), g.ctypes.data)


def test_symbol_is_bound():
    assert hasattr(_lib.lib(), "flgp_eigenpair_regression_objective")


@pytest.mark.parametrize("noise,approach,message", [
    (b"equal", b"posterior", "The noise setting is illegal!"),
    (b"", b"marginal", "The noise setting is illegal!"),
    (b"same", b"bayes", "This model selection approach is not supported!"),
    (b"different", b"Marginal", "This model selection approach is not supported!"),
])
def test_bad_strings_are_unsupported(noise, approach, message):
    assert _call(None, noise, approach) == -3
    assert _lib.lib().flgp_last_error().decode() == message


def test_null_pair_is_invalid():
    for noise, nx in ((b"same", 2), (b"different", 4)):
        for approach in (b"marginal", b"posterior"):
            assert _call(None, noise, approach, nx=nx) == -1


@pytest.mark.parametrize("noise", ["same", "different"])
@pytest.mark.parametrize("m", [8, 20], ids=["direct", "woodbury"])
def test_restatement_gradient_is_the_derivative(noise, m):
    """The unclipped gradient of the restatement against central differences of its own value (q = 2)."""
    rng = np.random.default_rng(11 + m)
    n, K, sigma = 60, 12, 1e-5
    values, V = R.synthetic_pair(n, K, rng)
    idx = rng.choice(n, m, replace=False)
    Y = rng.standard_normal((m, 2))
    x = np.r_[1.5, 0.3] if noise == "same" else np.r_[1.5, rng.uniform(0.1, 0.5, m)]
    _, g = R.nmll(values, V, K, idx, Y, x, sigma, noise, clip=False)
    fd = R.central_diff(lambda z: R.nmll(values, V, K, idx, Y, z, sigma, noise, clip=False)[0], x, 1e-5)
    assert np.abs(g - fd).max() <= 1e-6 * max(1.0, np.abs(g).max())
    # the posterior adds exact derivatives of its prior terms
    _, gp = R.objective(values, V, K, idx, Y, x, sigma, noise, "posterior", clip=False)
    fdp = R.central_diff(lambda z: R.objective(values, V, K, idx, Y, z, sigma, noise, "posterior", clip=False)[0], x, 1e-5)
    assert np.abs(gp - fdp).max() <= 1e-6 * max(1.0, np.abs(gp).max())
