"""CPU: the logit posterior's entry (flgp_eigenpair_logit_posterior, include/flgp_hip.h) refuses null pointers and shapes
below 1 before any device work, so these run without a GPU."""
import ctypes

import numpy as np
import pytest

from flgp_amd import _lib


def _call(ep=None, K=2, m=3, mnew=2, max_iter=100, idx0=True, Y=True, idx1=True, mean=True, cov=True):
    i0 = np.arange(max(m, 1), dtype=np.int32); i1 = np.arange(max(mnew, 1), dtype=np.int32)
    y = np.zeros(max(m, 1)); mu = np.zeros(max(mnew, 1)); cv = np.zeros(max(mnew, 1))
    it = ctypes.c_int()
    return _lib.lib().flgp_eigenpair_logit_posterior(ep, K, 1.0, 1e-3, 1e-3, i0.ctypes.data if idx0 else None, m,
                                                     y.ctypes.data if Y else None, i1.ctypes.data if idx1 else None, mnew, 1e-5,
                                                     max_iter, mu.ctypes.data if mean else None, cv.ctypes.data if cov else None,
                                                     ctypes.byref(it))


def test_symbol_is_bound():
    assert hasattr(_lib.lib(), "flgp_eigenpair_logit_posterior")
    assert "flgp_eigenpair_logit_posterior" in _lib.declared_symbols()


@pytest.mark.parametrize("missing", ["idx0", "Y", "idx1", "mean", "cov"])
def test_null_pointers_are_invalid(missing):
    assert _call() == -1                                   # the null pair
    assert _lib.lib().flgp_last_error().decode() == "logit_posterior: null pointer"
    assert _call(**{missing: False}) == -1
    assert _lib.lib().flgp_last_error().decode() == "logit_posterior: null pointer"


@pytest.mark.parametrize("kw", [dict(K=0), dict(K=-1), dict(m=0), dict(mnew=0), dict(max_iter=0)])
def test_shapes_below_one_are_invalid(kw):
    assert _call(**kw) == -1
    assert _lib.lib().flgp_last_error().decode().startswith("logit_posterior:")
