"""CPU: the batched Polya-Gamma entry (flgp_eigenpair_pg_predict_batch, include/flgp_hip.h) is declared,
exported and bound, and refuses bad arguments on the host before any device work -- pointers, shapes, values, then the
pair -- so these run without a GPU.  The Python wrappers refuse a bad column or t before they reach the library, with the
library's own text."""
import ctypes
import os
import re

import numpy as np
import pytest

from flgp_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "flgp_eigenpair_pg_predict_batch"
WHO = "eigenpair_pg_predict_batch"


def _p(a):
    return None if a is None else a.ctypes.data


def _call(B=2, m=3, mnew=2, ncol=2, n_sample=5, Y=None, col=None, ts=(1.0, 2.0), seeds=(7, 8), sigma=1e-3, sigma_nv=0.0,
          null=()):
    """The entry with a null pair and otherwise good arguments; ``null`` names the pointers to pass as NULL.  Returns
    (status, message)."""
    idx0 = np.arange(max(m, 1), dtype=np.int32); idx1 = np.arange(max(mnew, 1), dtype=np.int32)
    Ym = np.zeros((max(m, 1), max(ncol, 1)), order="F") if Y is None else np.asfortranarray(np.asarray(Y, dtype=np.float64))
    t = np.ascontiguousarray(np.asarray(ts, dtype=np.float64))
    sd = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64))
    cl = None if col is None else np.ascontiguousarray(np.asarray(col, dtype=np.int32))
    pi = np.zeros((max(mnew, 1), max(B, 1)), order="F")
    a = dict(idx0=idx0, Y=Ym, ts=t, seeds=sd, idx1=idx1, pi_pred=pi)
    for k in null:
        a[k] = None
    rc = _lib.lib().flgp_eigenpair_pg_predict_batch(None, 2, _p(a["idx0"]), m, _p(a["Y"]), ncol, _p(cl), _p(a["ts"]),
                                                    _p(a["seeds"]), B, float(sigma), float(sigma_nv), _p(a["idx1"]), mnew,
                                                    n_sample, 0, _p(a["pi_pred"]), None, None, None, None)
    return rc, _lib.lib().flgp_last_error().decode()


def test_symbol_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flgp_hip.h")).read(), flags=re.S)
    assert re.search(r"\b" + NAME + r"\s*\(", text)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    assert NAME in _lib.declared_symbols()
    assert hasattr(_lib.lib(), NAME)


@pytest.mark.parametrize("which", ["idx0", "Y", "ts", "seeds", "idx1", "pi_pred"])
def test_null_pointers(which):
    assert _call(null=(which,)) == (-1, WHO + ": null pointer")


@pytest.mark.parametrize("kw", [dict(B=0), dict(m=0), dict(mnew=0), dict(ncol=0)])
def test_bad_shapes(kw):
    a = dict(B=2, m=3, mnew=2, ncol=2); a.update(kw)
    rc, msg = _call(**kw)
    assert rc == -1
    assert msg == "%s: bad shape (B=%d, m=%d, m_new=%d, ncol=%d)" % (WHO, a["B"], a["m"], a["mnew"], a["ncol"])


def test_n_sample_below_one():
    assert _call(n_sample=0) == (-1, WHO + ": N_sample=0 must be at least 1")


def test_col_null_needs_one_column_per_chain():
    assert _call(ncol=3) == (-1, WHO + ": col may be NULL only if ncol == B (ncol=3, B=2)")


@pytest.mark.parametrize("col,text", [((0, 2), "chain 1 (t=2, seed=8): %s: col=2 is outside [0, ncol=2)" % WHO),
                                      ((-1, 0), "chain 0 (t=1, seed=7): %s: col=-1 is outside [0, ncol=2)" % WHO)])
def test_col_out_of_range_names_the_chain(col, text):
    assert _call(col=col) == (-1, text)


@pytest.mark.parametrize("t,text", [(float("nan"), "chain 1 (t=nan, seed=8): %s: t must be finite" % WHO),
                                    (float("inf"), "chain 1 (t=inf, seed=8): %s: t must be finite" % WHO)])
def test_bad_t_names_the_chain(t, text):
    assert _call(ts=(1.0, t)) == (-1, text)


@pytest.mark.parametrize("v", [1.5, -0.5, float("nan")])
def test_y_outside_the_unit_interval(v):
    Y = np.zeros((3, 2)); Y[2, 1] = v
    rc, msg = _call(Y=Y)
    assert rc == -1 and msg == "%s: Y[2, 1]=%g is outside [0, 1]" % (WHO, v)


@pytest.mark.parametrize("kw", [dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")),
                                dict(sigma_nv=float("nan")), dict(sigma_nv=float("inf"))])
def test_bad_sigma(kw):
    assert _call(**kw) == (-1, WHO + ": sigma must be finite and >= 0")


def test_null_pair_is_checked_last():
    assert _call() == (-1, WHO + ": null eigenpair")       # every other argument is good: the handle is what is refused
    assert _call(col=(1, 1)) == (-1, WHO + ": null eigenpair")


class NoLibrary:
    """A ResidentEigenPair whose handle is never used: the wrappers below must refuse before they reach the library."""
    _h = None
    test_pgbinary_batch = api.ResidentEigenPair.test_pgbinary_batch
    predict_logit_mult_gp_batch = api.ResidentEigenPair.predict_logit_mult_gp_batch


def _batch(*a, **kw):
    return NoLibrary().test_pgbinary_batch(*a, **kw)


def test_wrapper_refuses_like_the_library():
    idx0 = np.arange(3); idx1 = np.arange(2); Y = np.zeros((3, 2))
    for col, ts in (((0, 2), (1.0, 2.0)), ((-1, 0), (1.0, 2.0)), (None, (1.0, float("nan"))), ((1, 1), (1.0, float("inf")))):
        with pytest.raises(api.FlgpError) as e:
            _batch(idx0, idx1, 2, ts, Y, 1e-3, 0.0, col=col, seeds=(7, 8))
        rc, msg = _call(col=col, ts=ts)
        assert rc == e.value.code == -1 and e.value.message == msg and msg.startswith("chain ")
    with pytest.raises(api.FlgpError) as e:
        _batch(idx0, idx1, 2, (1.0, 2.0, 3.0), Y, 1e-3, 0.0, seed=1)
    assert e.value.message == _call(B=3, ts=(1.0, 2.0, 3.0), seeds=(1, 2, 3))[1]
    # the default seeds are seed + b
    with pytest.raises(api.FlgpError) as e:
        _batch(idx0, idx1, 2, (1.0, float("nan")), Y, 1e-3, 0.0, seed=41)
    assert e.value.message == "chain 1 (t=nan, seed=42): %s: t must be finite" % WHO


def test_multiclass_wrapper_refuses_bad_labels_and_t():
    idx0 = np.arange(3); idx1 = np.arange(2)
    for bad in ([0, 1, 2], [0, 0.5, 1], [0, -1, 1], [0, float("nan"), 1]):          # J = 2: labels 0 and 1
        with pytest.raises(api.FlgpError) as e:
            NoLibrary().predict_logit_mult_gp_batch(idx0, idx1, 2, [1.0, 2.0], bad, 1e-3, seed=1)
        assert e.value.code == -1 and "is not a class label in 0 .. 1" in e.value.message
    with pytest.raises(api.FlgpError) as e:
        NoLibrary().predict_logit_mult_gp_batch(idx0, idx1, 2, [1.0, float("inf")], [0, 1, 1], 1e-3, seed=5)
    assert e.value.message == "chain 1 (t=inf, seed=6): %s: t must be finite" % WHO
    with pytest.raises(ValueError):
        NoLibrary().predict_logit_mult_gp_batch(idx0, idx1, 2, [1.0, 2.0], [0, 1], 1e-3, seed=5)
