"""CPU: the Polya-Gamma entries (include/flgp_hip.h) are declared, exported and bound, and refuse bad
arguments before any device work, so these run without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from flgp_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("flgp_pg_draw", "flgp_pg_logit_predict", "flgp_eigenpair_pg_predict", "flgp_eigenpair_pg_predict_multiclass")


def _p(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data


def test_pg_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flgp_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(L, name), name
        assert name in _lib.declared_symbols(), name
    _lib.lib()


def _refused(rc, what):
    assert rc == -1, rc
    assert what in _lib.lib().flgp_last_error().decode()


@pytest.mark.parametrize("b,c,n,what", [
    (None, [0.5, np.nan], 2, "finite"),
    (None, [0.5, np.inf], 2, "finite"),
    ([1.0, 0.0], [0.5, 1.0], 2, "integer >= 1"),
    ([1.0, 1.5], [0.5, 1.0], 2, "integer >= 1"),
    ([1.0, -2.0], [0.5, 1.0], 2, "integer >= 1"),
    (None, [0.5], 0, "bad shape"),
])
def test_pg_draw_refusals(b, c, n, what):
    b = None if b is None else np.asarray(b, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    out = np.zeros(max(n, 1))
    _refused(_lib.lib().flgp_pg_draw(_p(b), _p(c), n, 1, _p(out)), what)
    _refused(_lib.lib().flgp_pg_draw(_p(b), None, n, 1, _p(out)), "null pointer")


def test_pgdraw_wrapper_refuses():
    with pytest.raises(api.FlgpError) as e:
        api.pgdraw(1, [0.0, np.nan], seed=1)
    assert e.value.code == -1
    with pytest.raises(api.FlgpError):
        api.pgdraw(0, [0.0, 1.0], seed=1)


@pytest.mark.parametrize("Y,n_sample,what", [
    ([0.0, 1.5, 1.0], 5, "outside [0, 1]"),
    ([0.0, -0.5, 1.0], 5, "outside [0, 1]"),
    ([0.0, np.nan, 1.0], 5, "outside [0, 1]"),
    ([0.0, 1.0, 1.0], 0, "N_sample"),
])
def test_pg_logit_predict_refusals(Y, n_sample, what):
    C = np.eye(3); Cnv = np.ones((2, 3), order="F"); Y = np.asarray(Y, dtype=np.float64)
    pi = np.zeros(2); y = np.zeros(2)
    _refused(_lib.lib().flgp_pg_logit_predict(_p(C), 3, _p(Y), _p(Cnv), 2, n_sample, 7, _p(pi), _p(y), None, None), what)
    with pytest.raises(api.FlgpError) as e:
        api.test_pgbinary_cpp(C, Y, Cnv, N_sample=n_sample, seed=7)
    assert e.value.code == -1


def test_pg_logit_predict_shapes_and_pointers():
    C = np.eye(3); Cnv = np.ones((2, 3), order="F"); Y = np.array([0.0, 1.0, 1.0])
    pi = np.zeros(2); y = np.zeros(2)
    L = _lib.lib()
    _refused(L.flgp_pg_logit_predict(_p(C), 0, _p(Y), _p(Cnv), 2, 5, 7, _p(pi), _p(y), None, None), "bad shape")
    _refused(L.flgp_pg_logit_predict(_p(C), 3, _p(Y), _p(Cnv), 0, 5, 7, _p(pi), _p(y), None, None), "bad shape")
    _refused(L.flgp_pg_logit_predict(None, 3, _p(Y), _p(Cnv), 2, 5, 7, _p(pi), _p(y), None, None), "null pointer")
    _refused(L.flgp_pg_logit_predict(_p(C), 3, _p(Y), _p(Cnv), 2, 5, 7, _p(pi), None, None, None), "null pointer")
    with pytest.raises(ValueError):
        api.test_pgbinary_cpp(C, Y[:2], Cnv)
    with pytest.raises(ValueError):
        api.test_pgbinary_cpp(C, Y, np.ones((2, 4)))


def _resident(t=1.0, sigma=1e-3, sigma_nv=0.0, Y=(0.0, 1.0, 1.0), m=3, mnew=2, n_sample=5, idx0=True):
    Y = np.asarray(Y, dtype=np.float64)
    i0 = np.arange(m, dtype=np.int32) if idx0 else None
    i1 = np.arange(mnew, dtype=np.int32)
    pi = np.zeros(max(mnew, 1)); y = np.zeros(max(mnew, 1))
    return _lib.lib().flgp_eigenpair_pg_predict(None, 2, float(t), float(sigma), float(sigma_nv), _p(i0), m, _p(Y), _p(i1), mnew,
                                                n_sample, 3, _p(pi), _p(y), None, None)


def test_eigenpair_pg_predict_refusals():
    _refused(_resident(t=np.nan), "t must be finite")
    _refused(_resident(t=np.inf), "t must be finite")
    _refused(_resident(sigma=-1.0), "sigma")
    _refused(_resident(sigma=np.nan), "sigma")
    _refused(_resident(sigma_nv=np.inf), "sigma")
    _refused(_resident(Y=(0.0, 2.0, 1.0)), "outside [0, 1]")
    _refused(_resident(n_sample=0), "N_sample")
    _refused(_resident(mnew=0), "bad shape")
    _refused(_resident(m=0, Y=(0.0,)), "bad shape")
    _refused(_resident(idx0=False), "null pointer")
    _refused(_resident(), "null eigenpair")       # every other argument is good: the handle is what is refused


def _multi(ts=(1.0, 2.0), Y=(0.0, 1.0, 1.0), n_sample=5, sigma=1e-3, J=None):
    ts = np.asarray(ts, dtype=np.float64); Y = np.asarray(Y, dtype=np.float64)
    J = ts.size if J is None else J
    i0 = np.arange(Y.size, dtype=np.int32); i1 = np.arange(2, dtype=np.int32)
    probs = np.zeros((2, max(J, 1)), order="F"); lab = np.zeros(2)
    return _lib.lib().flgp_eigenpair_pg_predict_multiclass(None, 2, _p(ts), J, float(sigma), _p(i0), Y.size, _p(Y), _p(i1), 2,
                                                           n_sample, 3, _p(probs), _p(lab))


def test_multiclass_refusals():
    _refused(_multi(ts=(1.0, np.nan)), "ts[1]")
    _refused(_multi(Y=(0.0, 1.5, 1.0)), "class label")
    _refused(_multi(Y=(0.0, -1.0, 1.0)), "class label")
    _refused(_multi(Y=(0.0, 2.0, 1.0)), "class label")      # J = 2 classes: labels 0 and 1
    _refused(_multi(n_sample=0), "N_sample")
    _refused(_multi(sigma=-1.0), "sigma")
    _refused(_multi(J=0, ts=(1.0,)), "bad shape")
    _refused(_multi(), "null eigenpair")
