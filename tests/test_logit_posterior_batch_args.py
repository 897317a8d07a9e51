"""CPU: the batched logit posterior's entry (flgp_eigenpair_logit_posterior_batch, include/flgp_hip.h) is
declared, exported and bound, and refuses bad arguments on the host before any device work -- pointers, shapes, columns
and t, sigmas, values, then the pair -- so these run without a GPU.  The Python wrapper refuses a bad column or t before it
reaches the library, with the library's own text."""
import ctypes
import os
import re

import numpy as np
import pytest

from flgp_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "flgp_eigenpair_logit_posterior_batch"
WHO = "logit_posterior_batch"


def _p(a):
    return None if a is None else a.ctypes.data


def _call(K=2, B=2, m=3, mnew=2, ncol=2, max_iter=100, Y=None, col=None, ts=(1.0, 2.0), s11=0.0, s22=1e-3, null=()):
    """The entry with a null pair and otherwise good arguments; ``null`` names the pointers to pass as NULL.  Returns
    (status, message)."""
    idx0 = np.arange(max(m, 1), dtype=np.int32); idx1 = np.arange(max(mnew, 1), dtype=np.int32)
    Ym = np.zeros((max(m, 1), max(ncol, 1)), order="F") if Y is None else np.asfortranarray(np.asarray(Y, dtype=np.float64))
    t = np.ascontiguousarray(np.asarray(ts, dtype=np.float64))
    cl = None if col is None else np.ascontiguousarray(np.asarray(col, dtype=np.int32))
    mean = np.zeros((max(mnew, 1), max(B, 1)), order="F"); cov = mean.copy()
    its = np.zeros(max(B, 1), dtype=np.int32)
    a = dict(idx0=idx0, Y=Ym, ts=t, idx1=idx1, mean=mean, cov=cov)
    for k in null:
        a[k] = None
    rc = _lib.lib().flgp_eigenpair_logit_posterior_batch(None, K, _p(a["idx0"]), m, _p(a["Y"]), ncol, _p(cl), _p(a["ts"]), B,
                                                         float(s11), float(s22), _p(a["idx1"]), mnew, 1e-5, max_iter, 0,
                                                         _p(a["mean"]), _p(a["cov"]), _p(its))
    return rc, _lib.lib().flgp_last_error().decode()


def test_symbol_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flgp_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint " + NAME + r"\s*\(", text)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    assert NAME in _lib.declared_symbols()
    assert hasattr(_lib.lib(), NAME)
    assert hasattr(api.ResidentEigenPair, "logit_posterior_batch")


@pytest.mark.parametrize("which", ["idx0", "Y", "ts", "idx1", "mean", "cov"])
def test_null_pointers(which):
    assert _call(null=(which,)) == (-1, WHO + ": null pointer")


@pytest.mark.parametrize("kw", [dict(K=0), dict(m=0), dict(mnew=0), dict(max_iter=0), dict(B=0), dict(ncol=0), dict(B=-1)])
def test_bad_shapes(kw):
    a = dict(K=2, m=3, mnew=2, max_iter=100, B=2, ncol=2); a.update(kw)
    rc, msg = _call(**kw)
    assert rc == -1
    assert msg == "%s: bad shape (K=%d, m=%d, m_new=%d, max_iter=%d, B=%d, ncol=%d)" % (
        WHO, a["K"], a["m"], a["mnew"], a["max_iter"], a["B"], a["ncol"])


def test_col_null_needs_one_column_per_problem():
    assert _call(ncol=3) == (-1, WHO + ": col may be NULL only if ncol == B (ncol=3, B=2)")
    assert _call(ncol=1) == (-1, WHO + ": col may be NULL only if ncol == B (ncol=1, B=2)")


@pytest.mark.parametrize("col,text", [((0, 2), "problem 1 (t=2): %s: col=2 is outside [0, ncol=2)" % WHO),
                                      ((-1, 0), "problem 0 (t=1): %s: col=-1 is outside [0, ncol=2)" % WHO)])
def test_col_out_of_range_names_the_problem(col, text):
    assert _call(col=col) == (-1, text)


@pytest.mark.parametrize("t,text", [(float("nan"), "problem 1 (t=nan): %s: t must be finite" % WHO),
                                    (float("inf"), "problem 1 (t=inf): %s: t must be finite" % WHO),
                                    (float("-inf"), "problem 1 (t=-inf): %s: t must be finite" % WHO)])
def test_bad_t_names_the_problem(t, text):
    assert _call(ts=(1.0, t)) == (-1, text)


@pytest.mark.parametrize("name,v", [("sigma11", -1.0), ("sigma11", float("nan")), ("sigma11", float("inf")),
                                    ("sigma22", -1e-3), ("sigma22", float("nan")), ("sigma22", float("inf"))])
def test_bad_sigma(name, v):
    kw = {"s11": v} if name == "sigma11" else {"s22": v}
    assert _call(**kw) == (-1, "%s: %s=%g must be finite and >= 0" % (WHO, name, v))


@pytest.mark.parametrize("v", [1.5, -0.5, float("nan")])
def test_y_outside_the_unit_interval(v):
    """the single entry's wording (check_labels with one trial per row), the row counted within its column"""
    Y = np.zeros((3, 2)); Y[2, 1] = v
    rc, msg = _call(Y=Y)
    assert rc == -1 and msg == "%s: Y[2]=%g is outside [0, N[2]=1]" % (WHO, v)


def test_null_pair_is_checked_last():
    assert _call() == (-1, WHO + ": null pointer")         # every other argument is good: the handle is what is refused
    assert _call(col=(1, 1)) == (-1, WHO + ": null pointer")
    # ... and everything above is refused before it: none of these messages is the pair's
    assert "bad shape" in _call(B=0)[1] and "col may be NULL" in _call(ncol=3)[1] and "sigma11" in _call(s11=-1.0)[1]


class NoLibrary:
    """A ResidentEigenPair whose handle is never used: the wrapper below must refuse before it reaches the library."""
    _h = None
    logit_posterior_batch = api.ResidentEigenPair.logit_posterior_batch


def _batch(*a, **kw):
    return NoLibrary().logit_posterior_batch(*a, **kw)


def test_wrapper_refuses_like_the_library():
    idx0 = np.arange(3); idx1 = np.arange(2); Y = np.zeros((3, 2))
    for col, ts in (((0, 2), (1.0, 2.0)), ((-1, 0), (1.0, 2.0)), (None, (1.0, float("nan"))), ((1, 1), (1.0, float("inf")))):
        with pytest.raises(api.FlgpError) as e:
            _batch(idx0, idx1, 2, ts, Y, col=col)
        rc, msg = _call(col=col, ts=ts)
        assert rc == e.value.code == -1 and e.value.message == msg and msg.startswith("problem ")
    with pytest.raises(api.FlgpError) as e:
        _batch(idx0, idx1, 2, (1.0, 2.0, 3.0), Y)
    assert e.value.message == _call(B=3, ts=(1.0, 2.0, 3.0))[1]
    with pytest.raises(ValueError, match="one row per entry of idx0"):
        _batch(idx0, idx1, 2, (1.0, 2.0), np.zeros((4, 2)))
    with pytest.raises(ValueError, match="one entry per value of t"):
        _batch(idx0, idx1, 2, (1.0, 2.0), Y, col=(0, 1, 1))
