"""CPU: the logit training objective's entry (flgp_eigenpair_logit_objective, include/flgp_hip.h) checks its approach
string before anything else, and its pointers before any device work."""
import ctypes

import numpy as np
import pytest

from flgp_amd import _lib


def _call(ep, approach, m=3, K=2):
    idx = np.arange(m, dtype=np.int32)
    Y = np.zeros(m)
    v = ctypes.c_double()
    it = ctypes.c_int()
    return _lib.lib().flgp_eigenpair_logit_objective(ep, K, idx.ctypes.data, m, Y.ctypes.data, None, 1e-3, approach, None,
                                                     1.0, 1e-5, 100, ctypes.byref(v), ctypes.byref(it))


def test_symbol_is_bound():
    assert hasattr(_lib.lib(), "flgp_eigenpair_logit_objective")


@pytest.mark.parametrize("approach", [b"bayes", b"Marginal", b"posterior ", b""])
def test_bad_approach_is_unsupported(approach):
    assert _call(None, approach) == -3
    assert _lib.lib().flgp_last_error().decode() == "This model selection approach is not supported!"


def test_null_pointers_are_invalid():
    for approach in (b"marginal", b"posterior"):
        assert _call(None, approach) == -1
    assert _call(None, None) == -1
