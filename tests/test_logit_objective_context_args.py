"""CPU: the logit training context (flgp_logit_batch_*, include/flgp_hip.h) refuses its approach string before
anything else and its pointers and counts before any device work; the Python context refuses a wrong-length ts, a problem
number out of range and a bad t before it reaches the library, with the library's texts."""
import ctypes
import os

import numpy as np
import pytest

from flgp_amd import _lib, api

SYMBOLS = ["flgp_logit_batch_create", "flgp_logit_batch_dims", "flgp_logit_batch_eval", "flgp_logit_batch_free"]
WHO = "logit_objective_context"


def _create(approach, eps=False, col=None, B=2, K=2, idx=True, m=3, Y=True, ncol=2, out=True, max_iter=100, sigma=1e-3):
    rows = np.arange(m, dtype=np.int32)
    Ym = np.zeros((max(m, 1), max(ncol, 1)), order="F")
    arr = (ctypes.c_void_p * 2)(None, None)
    cols = None if col is None else np.asarray(col, dtype=np.int32)
    h = ctypes.c_void_p()
    return _lib.lib().flgp_logit_batch_create(arr if eps else None, None if cols is None else cols.ctypes.data, B, K,
                                              rows.ctypes.data if idx else None, m, Ym.ctypes.data if Y else None, ncol,
                                              None, sigma, approach, None, 1e-5, max_iter, 0,
                                              ctypes.byref(h) if out else None)


def _error():
    return _lib.lib().flgp_last_error().decode()


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbols_are_bound_and_declared(name):
    assert hasattr(_lib.lib(), name)
    assert name in _lib.declared_symbols()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "flgp_hip.h")) as f:
        header = f.read()
    assert name + "(" in header


@pytest.mark.parametrize("approach", [b"bayes", b"Marginal", b""])
def test_a_bad_approach_is_unsupported_before_the_null_checks(approach):
    assert _create(approach, idx=False, Y=False, out=False) == -3
    assert _error() == "This model selection approach is not supported!"


def test_create_refuses_null_pointers_and_bad_counts():
    for approach in (b"marginal", b"posterior"):
        assert _create(approach) == -1                                   # eps
        assert _error() == WHO + ": null pointer"
        assert _create(approach, eps=True, idx=False) == -1
        assert _create(approach, eps=True, Y=False) == -1
        assert _create(approach, eps=True, out=False) == -1
        assert _error() == WHO + ": null pointer"
        for bad in (dict(B=0), dict(K=0), dict(m=0), dict(ncol=0), dict(max_iter=0)):
            assert _create(approach, eps=True, **bad) == -1, bad
            assert "bad shape" in _error(), bad
        assert _create(approach, eps=True, ncol=3) == -1                 # col NULL with ncol != B
        assert _error() == WHO + ": col may be NULL only if ncol == B (ncol=3, B=2)"
    assert _create(None) == -1
    assert _error() == WHO + ": null pointer"


def test_a_null_pair_is_named_as_its_problem():
    assert _create(b"marginal", eps=True) == -1
    assert _error() == "problem 0: %s: null pointer" % WHO
    assert _create(b"posterior", eps=True, col=[0, 1], ncol=5) == -1
    assert _error() == "problem 0: %s: null pointer" % WHO


def test_eval_and_dims_refuse_a_null_handle_and_free_takes_one():
    L = _lib.lib()
    t = np.ones(1); v = np.zeros(1)
    assert L.flgp_logit_batch_eval(None, None, 1, t.ctypes.data, v.ctypes.data, None, None) == -1
    assert _error() == WHO + ": null pointer"
    assert L.flgp_logit_batch_dims(None, None, None, None, None, None, None) == -1
    assert _error() == WHO + ": null pointer"
    L.flgp_logit_batch_free(None)


def _context(B=3, approach="posterior"):
    """A context whose handle is never used: the checks below must refuse before they reach the library."""
    ctx = object.__new__(api.LogitObjectiveBatch)
    ctx._h = None
    ctx._pairs = []
    ctx._set(B, 2, 4, 3, approach)
    return ctx


def test_wrapper_refuses_a_wrong_length_ts():
    with pytest.raises(api.FlgpError) as e:
        _context()(np.ones(2))                                          # prob None with A != B
    assert e.value.code == -1
    assert e.value.message == WHO + ": prob may be NULL only if A == B (A=2, B=3)"
    with pytest.raises(api.FlgpError) as e:
        _context()(np.ones(0), prob=[])
    assert e.value.message == WHO + ": A=0 problems"
    with pytest.raises(ValueError):
        _context()(np.ones(2), prob=[0, 1, 2])


def test_wrapper_refuses_a_problem_out_of_range():
    for bad in (3, -1):
        with pytest.raises(api.FlgpError) as e:
            _context()(np.array([1.0, 2.5]), prob=[2, bad])
        assert e.value.code == -1
        assert e.value.message == "position 1 (t=2.5): %s: prob=%d is outside [0, B=3)" % (WHO, bad)


@pytest.mark.parametrize("t,text", [
    (np.nan, "position 2 (t=nan): %s: t must be finite" % WHO),
    (np.inf, "position 2 (t=inf): %s: t must be finite" % WHO),
    (0.0, 'position 2 (t=0): %s: t must be positive under "posterior"' % WHO),
    (-1.5, 'position 2 (t=-1.5): %s: t must be positive under "posterior"' % WHO),
])
def test_wrapper_refuses_a_bad_t(t, text):
    with pytest.raises(api.FlgpError) as e:
        _context()(np.array([1.0, 2.0, t]))
    assert e.value.code == -1 and e.value.message == text


def test_the_position_is_checked_in_the_librarys_order():
    """prob before t, and the lowest position first"""
    with pytest.raises(api.FlgpError) as e:
        _context()(np.array([1.0, np.inf, -1.0]), prob=[0, 7, 1])
    assert e.value.message == "position 1 (t=inf): %s: prob=7 is outside [0, B=3)" % WHO


def test_wrapper_takes_t_zero_under_marginal_as_far_as_the_library():
    """t <= 0 is refused under "posterior" only: under "marginal" the checks pass"""
    ts, prob = _context(B=1, approach="marginal")._checked([0.0], None)
    assert prob is None and ts.shape == (1,)
    ts, prob = _context(B=2, approach="marginal")._checked([-1.0, 3.0, 2.0], [1, 1, 0])
    assert prob.dtype == np.int32 and ts.dtype == np.float64
