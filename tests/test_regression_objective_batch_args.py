"""CPU: the batched regression training objective's context (flgp_regression_batch_*, include/flgp_hip.h)
refuses its strings before anything else and its pointers and counts before any device work; the Python context refuses a
wrong-shaped X, a problem number out of range and a bad x before it reaches the library, with the library's texts."""
import ctypes
import os

import numpy as np
import pytest

from flgp_amd import _lib, api

SYMBOLS = ["flgp_regression_batch_create", "flgp_regression_batch_dims", "flgp_regression_batch_eval",
           "flgp_regression_batch_free"]


def _create(noise, approach, eps=False, B=2, idx=True, Y=True, out=True, m=3, K=2):
    rows = np.arange(m, dtype=np.int32)
    Ym = np.zeros(m)
    arr = (ctypes.c_void_p * 2)(None, None)
    h = ctypes.c_void_p()
    return _lib.lib().flgp_regression_batch_create(arr if eps else None, B, K, rows.ctypes.data if idx else None, m,
                                                   Ym.ctypes.data if Y else None, 1, 1e-5, noise, approach, None, 0,
                                                   ctypes.byref(h) if out else None)


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbols_are_bound_and_declared(name):
    assert hasattr(_lib.lib(), name)
    assert name in _lib.declared_symbols()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "flgp_hip.h")) as f:
        header = f.read()
    assert name + "(" in header


@pytest.mark.parametrize("noise,approach,message", [
    (b"equal", b"posterior", "The noise setting is illegal!"),
    (b"", b"marginal", "The noise setting is illegal!"),
    (b"same", b"bayes", "This model selection approach is not supported!"),
    (b"different", b"Marginal", "This model selection approach is not supported!"),
])
def test_bad_strings_are_unsupported_before_the_null_checks(noise, approach, message):
    assert _create(noise, approach, idx=False, Y=False, out=False) == -3
    assert _lib.lib().flgp_last_error().decode() == message


def test_create_refuses_null_pointers_and_empty_batches():
    for noise in (b"same", b"different"):
        for approach in (b"marginal", b"posterior"):
            assert _create(noise, approach) == -1                       # eps
            assert "null pointer" in _lib.lib().flgp_last_error().decode()
            assert _create(noise, approach, eps=True, idx=False) == -1
            assert _create(noise, approach, eps=True, Y=False) == -1
            assert _create(noise, approach, eps=True, out=False) == -1
            assert _create(noise, approach, eps=True, B=0) == -1
            assert _create(noise, approach, eps=True) == -1             # eps[0] is null
            assert _lib.lib().flgp_last_error().decode() == "problem 0: regression_objective_batch: null pointer"
    assert _create(None, b"marginal") == -1
    assert _create(b"same", None) == -1


def test_eval_and_dims_refuse_a_null_handle():
    L = _lib.lib()
    x = np.ones(2); v = np.zeros(1)
    assert L.flgp_regression_batch_eval(None, None, 1, x.ctypes.data, 2, v.ctypes.data, None, 2, None) == -1
    assert "null pointer" in L.flgp_last_error().decode()
    assert L.flgp_regression_batch_dims(None, None, None, None, None, None, None) == -1
    L.flgp_regression_batch_free(None)


def _context(B=3, m=4, noise="same", approach="posterior", sigma=1e-5):
    """A context whose handle is never used: the checks below must refuse before they reach the library."""
    ctx = object.__new__(api.RegressionObjectiveBatch)
    ctx._h = None
    ctx._pairs = []
    ctx._set(B, 2, m, 1, sigma, noise, approach)
    return ctx


def test_wrapper_refuses_a_wrong_shaped_x():
    with pytest.raises(api.FlgpError) as e:
        _context()(np.ones((3, 3)))
    assert e.value.code == -1
    assert e.value.message == 'regression_objective_batch: noise "same" takes 2 parameters, not 3'
    with pytest.raises(api.FlgpError) as e:
        _context(noise="different")(np.ones((3, 2)))
    assert e.value.message == 'regression_objective_batch: noise "different" takes 5 parameters, not 2'
    with pytest.raises(api.FlgpError) as e:
        _context()(np.ones((2, 2)))                                    # prob None with A != B
    assert e.value.message == "regression_objective_batch: prob may be NULL only if A == B (A=2, B=3)"
    with pytest.raises(api.FlgpError) as e:
        _context()(np.ones((0, 2)), prob=[])
    assert e.value.message == "regression_objective_batch: A=0 problems"
    with pytest.raises(ValueError):
        _context()(np.ones((2, 2)), prob=[0, 1, 2])


def test_wrapper_refuses_a_problem_out_of_range():
    for bad in (3, -1):
        with pytest.raises(api.FlgpError) as e:
            _context()(np.ones((2, 2)), prob=[2, bad])
        assert e.value.code == -1
        assert e.value.message == "position 1: regression_objective_batch: prob=%d is outside [0, B=3)" % bad


@pytest.mark.parametrize("x,text", [
    ([1.0, np.nan], "position 2: regression_objective_batch: x must be finite"),
    ([np.inf, 0.2], "position 2: regression_objective_batch: x must be finite"),
    ([1.0, -1e-5], "position 2: regression_objective_batch: x[1] + sigma must be positive"),
    ([0.0, 0.2], 'position 2: regression_objective_batch: t = x[0] must be positive under "posterior"'),
])
def test_wrapper_refuses_a_bad_x(x, text):
    X = np.array([[1.0, 0.2], [2.0, 0.3], x])
    with pytest.raises(api.FlgpError) as e:
        _context()(X)
    assert e.value.code == -1 and e.value.message == text


def test_wrapper_takes_t_zero_under_marginal_as_far_as_the_library():
    """t <= 0 is refused under "posterior" only: under "marginal" the checks pass (and the missing handle is reached)."""
    X = np.array([[0.0, 0.2]])
    ctx = _context(B=1, approach="marginal")
    Xc, prob = ctx._checked(X, None)
    assert prob is None and Xc.shape == (1, 2)
