"""CPU: the batched logit training objective's entry (flgp_eigenpair_logit_objective_batch, include/flgp_hip.h) checks its
approach string before anything else and its pointers and counts before any device work; the Python wrappers refuse a bad
column, a bad t and a wrong-shaped ts before they call the library, with the library's message texts."""
import ctypes

import numpy as np
import pytest

from flgp_amd import _lib, api


def _call(ep, approach, m=3, K=2, B=2, ncol=2, Y=True, ts=True, values=True):
    idx = np.arange(m, dtype=np.int32)
    Ym = np.zeros((m, max(ncol, 1)), order="F")
    t = np.ones(max(B, 1))
    v = np.zeros(max(B, 1)); it = np.zeros(max(B, 1), dtype=np.int32)
    return _lib.lib().flgp_eigenpair_logit_objective_batch(ep, K, idx.ctypes.data, m, Ym.ctypes.data if Y else None, ncol, None,
                                                           None, t.ctypes.data if ts else None, B, 1e-3, approach, None, 1e-5,
                                                           100, 0, v.ctypes.data if values else None, it.ctypes.data)


def test_symbol_is_bound():
    assert hasattr(_lib.lib(), "flgp_eigenpair_logit_objective_batch")
    assert "flgp_eigenpair_logit_objective_batch" in _lib.declared_symbols()


@pytest.mark.parametrize("approach", [b"bayes", b"Marginal", b"posterior ", b""])
def test_bad_approach_is_unsupported_before_the_null_checks(approach):
    assert _call(None, approach, Y=False, ts=False, values=False) == -3
    assert _lib.lib().flgp_last_error().decode() == "This model selection approach is not supported!"


def test_null_pointers_and_empty_batches_are_invalid():
    for approach in (b"marginal", b"posterior"):
        assert _call(None, approach) == -1
        assert _call(None, approach, B=0) == -1
        assert _call(None, approach, ncol=0) == -1
        assert "null pointer" in _lib.lib().flgp_last_error().decode()
    assert _call(None, None) == -1


class NoLibrary:
    """A ResidentEigenPair whose handle is never used: the wrappers below must refuse before they reach the library."""
    _h = None
    logit_objective_batch = api.ResidentEigenPair.logit_objective_batch
    logit_objective_multiclass = api.ResidentEigenPair.logit_objective_multiclass


def _batch(*a, **kw):
    return NoLibrary().logit_objective_batch(*a, **kw)


def _multi(*a, **kw):
    return NoLibrary().logit_objective_multiclass(*a, **kw)


def test_wrapper_refuses_a_column_out_of_range():
    idx = np.arange(4); Y = np.zeros((4, 3))
    with pytest.raises(api.FlgpError) as e:
        _batch([1.0, 2.5, 4.0], 2, idx, Y, col=[0, 3, 1])
    assert e.value.code == -1
    assert e.value.message == "problem 1 (t=2.5): logit_objective_batch: col=3 is outside [0, ncol=3)"
    with pytest.raises(api.FlgpError) as e:
        _batch([1.0, 2.5], 2, idx, Y, col=[-1, 0])
    assert e.value.message == "problem 0 (t=1): logit_objective_batch: col=-1 is outside [0, ncol=3)"


def test_wrapper_refuses_col_none_with_another_column_count():
    with pytest.raises(api.FlgpError) as e:
        _batch([1.0, 2.0], 2, np.arange(4), np.zeros((4, 3)))
    assert e.value.code == -1
    assert e.value.message == "logit_objective_batch: col may be NULL only if ncol == B (ncol=3, B=2)"


@pytest.mark.parametrize("t,text", [(float("nan"), "problem 2 (t=nan): logit_objective_batch: t must be finite"),
                                    (float("inf"), "problem 2 (t=inf): logit_objective_batch: t must be finite"),
                                    (0.0, 'problem 2 (t=0): logit_objective_batch: t must be positive under "posterior"')])
def test_wrapper_refuses_a_bad_t(t, text):
    with pytest.raises(api.FlgpError) as e:
        _batch([1.0, 2.0, t], 2, np.arange(4), np.zeros((4, 3)))
    assert e.value.code == -1 and e.value.message == text


def test_multiclass_wrapper_refuses_a_wrong_shaped_ts_and_bad_labels():
    idx = np.arange(6); labels = np.array([0, 1, 2, 2, 1, 0])
    for ts in ([1.0, 2.0], np.ones((2, 3)), np.ones((3, 2, 2)), 1.0):
        with pytest.raises(ValueError):
            _multi(ts, 2, idx, labels)
    for bad in ([0, 1, 2.5, 2, 1, 0], [0, 1, -1, 2, 1, 0], [0, 1, np.nan, 2, 1, 0]):
        with pytest.raises(ValueError):
            _multi([1.0, 2.0, 3.0], 2, idx, bad)
    # a bad t inside a J x T profile is refused with the problem named: class 1, second point = problem 3
    ts = np.ones((3, 2)); ts[1, 1] = np.nan
    with pytest.raises(api.FlgpError) as e:
        _multi(ts, 2, idx, labels)
    assert e.value.message == "problem 3 (t=nan): logit_objective_batch: t must be finite"
