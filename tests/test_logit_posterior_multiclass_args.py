"""CPU: the one-vs-rest logit posterior's two entries (flgp_eigenpair_logit_posterior_multiclass and its _nll variant,
include/flgp_hip.h) are declared, bound and refuse what needs no pair -- J < 1 and null pointers -- before any device work;
the Python method checks its array lengths before it touches the library."""
import ctypes
import os
import re

import numpy as np
import pytest

from flgp_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["flgp_eigenpair_logit_posterior_multiclass", "flgp_eigenpair_logit_posterior_multiclass_nll"]


def _call(nll, J=3, ep=None, out=True):
    m, mnew = 4, 2
    i0 = np.arange(m, dtype=np.int32); i1 = np.arange(mnew, dtype=np.int32)
    ts = np.ones(max(J, 1)); y = np.zeros(m); mu = np.zeros((mnew, max(J, 1)), order="F"); cv = mu.copy()
    head = (ep, 2, ts.ctypes.data, J, 0.0, 1e-3, i0.ctypes.data, m, y.ctypes.data, i1.ctypes.data, mnew, 1e-5, 100, 4,
            mu.ctypes.data, cv.ctypes.data, None)
    if not nll:
        return _lib.lib().flgp_eigenpair_logit_posterior_multiclass(*head)
    tg = np.zeros(mnew); val = ctypes.c_double()
    return _lib.lib().flgp_eigenpair_logit_posterior_multiclass_nll(*head, tg.ctypes.data, 10, 1, ctypes.byref(val) if out else None)


def test_symbols_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "flgp_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in _lib.declared_symbols() and hasattr(_lib.lib(), name)


@pytest.mark.parametrize("nll", [False, True])
def test_refusals_that_need_no_pair(nll):
    assert _call(nll, J=0) == -1
    assert _lib.lib().flgp_last_error().decode() == "logit_posterior_multiclass: J=0 must be at least 1"
    assert _call(nll, J=-2) == -1
    assert _lib.lib().flgp_last_error().decode() == "logit_posterior_multiclass: J=-2 must be at least 1"
    assert _call(nll) == -1                                   # the null pair
    assert _lib.lib().flgp_last_error().decode() == "logit_posterior_multiclass: null pointer"


def test_the_score_needs_somewhere_to_go():
    assert _call(True, out=False) == -1
    assert _lib.lib().flgp_last_error().decode() == "logit_posterior_multiclass: null pointer"


def test_python_method_checks_lengths_before_the_library():
    rp = object.__new__(api.ResidentEigenPair)                # no handle: reaching the library would fail on it
    idx0, idx1, Y = np.arange(6), np.arange(10, 14), np.array([0, 1, 2, 0, 1, 2.0])
    with pytest.raises(ValueError, match="one entry per row of idx0"):
        rp.logit_posterior_multiclass(idx0, idx1, 2, [1.0, 2.0, 3.0], Y[:5], 1e-3)
    with pytest.raises(ValueError, match="one t per class"):
        rp.logit_posterior_multiclass(idx0, idx1, 2, [1.0, 2.0], Y, 1e-3, target=[0, 1, 2, 1])
    with pytest.raises(ValueError, match="one entry per row of idx1"):
        rp.logit_posterior_multiclass(idx0, idx1, 2, [1.0, 2.0, 3.0], Y, 1e-3, target=[0, 1, 2])
    with pytest.raises(ValueError, match="needs a target"):
        rp.logit_posterior_multiclass(idx0, idx1, 2, [1.0, 2.0, 3.0], Y, 1e-3, return_posterior=False)
