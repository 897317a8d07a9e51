"""CPU: the fitted-predictor entries (include/flgp_hip.h) are declared, exported and bound, and every
refusal made before any device work arrives with FLGP_ERR_INVALID and the documented name, *out cleared; so these run
without a GPU (the refusals that need live handles -- a pair of another fit, ep->K != the model's K, a NaN in X -- are in
tests/test_gpu_predictor.py).  The Python class checks its arrays before it touches the library."""
import ctypes
import os
import re

import numpy as np
import pytest

from flgp_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("flgp_predictor_regression_create", "flgp_predictor_logit_create", "flgp_predictor_dims", "flgp_predictor_to_host",
         "flgp_predictor_apply", "flgp_dev_predictor_apply", "flgp_predictor_free", "flgp_dev_predictor_rows")
FAKE = 8               # a non-null handle: every refusal here comes before a handle is looked at


def _message():
    return _lib.lib().flgp_last_error().decode()


def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flgp_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(L, name), name
        assert name in _lib.declared_symbols(), name
    assert re.search(r"typedef\s+struct\s+flgp_predictor\s+flgp_predictor\s*;", text)
    for method in ("regression", "logit", "apply", "to_host", "free"):
        assert callable(getattr(api.Predictor, method))


def _regression(model=FAKE, ep=FAKE, K=2, m=3, q=1, n_noise=1, t=1.0, sigma=1e-3, idx0=True, Y=True, noise=True, out="byref"):
    i0 = np.arange(max(m, 1), dtype=np.int32); y = np.zeros((max(m, 1), max(q, 1)), order="F"); nz = np.full(max(m, 1), 0.1)
    h = ctypes.c_void_p(1)
    rc = _lib.lib().flgp_predictor_regression_create(model, ep, K, i0.ctypes.data if idx0 else None, m, y.ctypes.data if Y else None,
                                                     q, t, nz.ctypes.data if noise else None, n_noise, sigma,
                                                     ctypes.byref(h) if out else None)
    return rc, h.value


REGRESSION_REFUSALS = [
    (dict(model=None), "predictor_regression: null model"),
    (dict(K=0), "predictor_regression: bad shape"), (dict(m=0), "predictor_regression: bad shape"),
    (dict(q=0), "predictor_regression: bad shape"), (dict(m=-3), "predictor_regression: bad shape"),
    (dict(n_noise=2), 'predictor_regression: n_noise=2 must be 1 ("same") or m=3 ("different")'),
    (dict(n_noise=0), "predictor_regression: n_noise=0"),
    (dict(t=float("nan")), "predictor_regression: t=nan"), (dict(sigma=float("inf")), "must be finite"),
    (dict(ep=None), "predictor_regression: null pointer"), (dict(idx0=False), "predictor_regression: null pointer"),
    (dict(Y=False), "predictor_regression: null pointer"), (dict(noise=False), "predictor_regression: null pointer"),
]


@pytest.mark.parametrize("kw,text", REGRESSION_REFUSALS)
def test_regression_create_refuses_before_any_device_work(kw, text):
    rc, h = _regression(**kw)
    assert rc == -1 and text in _message(), _message()
    assert h is None                                           # *out is cleared on every refusal


def test_create_without_out_is_a_null_pointer():
    assert _regression(out=None)[0] == -1 and _message() == "predictor_regression: null pointer"
    assert _logit(out=None)[0] == -1 and _message() == "predictor_logit: null pointer"


def _logit(model=FAKE, ep=FAKE, K=2, m=3, ncol=2, col=(0, 1), ts=(1.0, 2.0), B=None, sigma11=0.0, sigma22=1e-3, max_iter=10,
           idx0=True, Y=True, y_value=1.0, out="byref"):
    i0 = np.arange(max(m, 1), dtype=np.int32); y = np.full((max(m, 1), max(ncol, 1)), y_value, order="F")
    tsa = np.array(ts, dtype=np.float64) if ts is not None else None
    cols = np.array(col, dtype=np.int32) if col is not None else None
    B = (len(ts) if ts is not None else 1) if B is None else B
    h = ctypes.c_void_p(1)
    rc = _lib.lib().flgp_predictor_logit_create(model, ep, K, i0.ctypes.data if idx0 else None, m, y.ctypes.data if Y else None, ncol,
                                                cols.ctypes.data if cols is not None else None,
                                                tsa.ctypes.data if tsa is not None else None, B, sigma11, sigma22, 1e-5, max_iter, 0,
                                                None, ctypes.byref(h) if out else None)
    return rc, h.value


LOGIT_REFUSALS = [
    (dict(model=None), "predictor_logit: null model"),
    (dict(idx0=False), "predictor_logit: null pointer"), (dict(Y=False), "predictor_logit: null pointer"),
    (dict(ts=None), "predictor_logit: null pointer"),
    (dict(K=0), "predictor_logit: bad shape"), (dict(m=0), "predictor_logit: bad shape"),
    (dict(max_iter=0), "predictor_logit: bad shape"), (dict(B=0), "predictor_logit: bad shape"),
    (dict(ncol=0), "predictor_logit: bad shape"),
    (dict(col=None, ncol=3), "predictor_logit: col may be NULL only if ncol == B (ncol=3, B=2)"),
    (dict(col=(0, 2)), "problem 1 (t=2): predictor_logit: col=2 is outside [0, ncol=2)"),
    (dict(ts=(1.0, float("inf"))), "problem 1 (t=inf): predictor_logit: t must be finite"),
    (dict(sigma11=-1.0), "predictor_logit: sigma11=-1 must be finite and >= 0"),
    (dict(sigma22=float("nan")), "predictor_logit: sigma22=nan must be finite and >= 0"),
    (dict(y_value=1.5), "predictor_logit"),
    (dict(ep=None), "predictor_logit: null pointer"),
]


@pytest.mark.parametrize("kw,text", LOGIT_REFUSALS)
def test_logit_create_refuses_before_any_device_work(kw, text):
    rc, h = _logit(**kw)
    assert rc == -1 and text in _message(), _message()
    assert h is None


def test_apply_dims_to_host_and_free():
    L = _lib.lib()
    X = np.zeros((5, 3), order="F"); v = np.zeros(5)
    for args, text in (((None, None, 5, v.ctypes.data, v.ctypes.data), "predictor_apply: null pointer"),
                       ((None, X.ctypes.data, 5, None, None), "predictor_apply: null pointer"),
                       ((None, X.ctypes.data, 0, v.ctypes.data, None), "predictor_apply: need n_new >= 1 (n_new=0)"),
                       ((None, X.ctypes.data, 5, v.ctypes.data, v.ctypes.data), "predictor_apply: null handle")):
        assert L.flgp_predictor_apply(*args) == -1 and _message() == text
    for args, text in (((None, None, None, 5, 5, v.ctypes.data, 5, v.ctypes.data, 5), "null pointer"),
                       ((None, None, X.ctypes.data, 5, 5, None, 5, None, 5), "null pointer"),
                       ((None, None, X.ctypes.data, 0, 5, v.ctypes.data, 5, None, 5), "n_new >= 1"),
                       ((None, None, X.ctypes.data, 5, 4, v.ctypes.data, 5, None, 5), "leading dimension"),
                       ((None, None, X.ctypes.data, 5, 5, v.ctypes.data, 4, None, 5), "leading dimension"),
                       ((None, None, X.ctypes.data, 5, 5, None, 5, v.ctypes.data, 4), "leading dimension"),
                       ((None, None, X.ctypes.data, 5, 5, v.ctypes.data, 5, v.ctypes.data, 5), "null handle")):
        assert L.flgp_dev_predictor_apply(*args) == -1 and text in _message() and _message().startswith("predictor_apply")
    assert L.flgp_predictor_dims(None, *[None] * 8) == -1 and _message() == "predictor_dims: null handle"
    assert L.flgp_predictor_to_host(None, None, None) == -1 and _message() == "predictor_to_host: null handle"
    L.flgp_predictor_free(None)                                # like free(NULL)


def _rows(idx=FAKE, val=FAKE, n=4, r=2, P=FAKE, ldp=8, s=5, groups=2, K=3, q=1, cg=FAKE, mean=FAKE, ldm=4, var=FAKE, ldv=4):
    return _lib.lib().flgp_dev_predictor_rows(None, idx, val, n, r, P, ldp, s, groups, K, q, cg, mean, ldm, var, ldv)


ROWS_REFUSALS = [
    (dict(idx=None), "null pointer"), (dict(val=None), "null pointer"), (dict(P=None), "null pointer"),
    (dict(mean=None, var=None), "null pointer (no output is wanted)"), (dict(cg=None), "null pointer (the variance needs cg)"),
    (dict(n=0), "bad shape"), (dict(r=0), "bad shape"), (dict(r=33), "bad shape"), (dict(s=0), "bad shape"),
    (dict(groups=0), "bad shape"), (dict(K=0), "bad shape"), (dict(q=-1), "bad shape"),
    (dict(q=0), "a mean needs q >= 1"),
    (dict(ldp=7), "ldp=7 is below groups (K + q) = 8"),
    (dict(ldm=3), "leading dimension"), (dict(ldv=3), "leading dimension"),
]


@pytest.mark.parametrize("kw,text", ROWS_REFUSALS)
def test_row_kernel_refuses_before_any_launch(kw, text):
    assert _rows(**kw) == -1
    assert _message().startswith("predictor_rows: ") and text in _message(), _message()


class _Pair:
    def __init__(self, handle=ctypes.c_void_p(0)):
        self._h = handle


def test_python_class_checks_before_the_library():
    model = api.SpectrumModel(ctypes.c_void_p(0), dims=(100, 3, 10, 3, 4, 0, 2, 1))
    idx0, Y = np.arange(6), np.zeros((6, 2))
    with pytest.raises(TypeError, match="SpectrumModel"):
        api.Predictor.regression(object(), _Pair(), Y, idx0, 2, (1.0, 0.1), 1e-3)
    with pytest.raises(ValueError, match="pair has been freed"):
        api.Predictor.regression(model, _Pair(None), Y, idx0, 2, (1.0, 0.1), 1e-3)
    with pytest.raises(ValueError, match="one row per entry of idx0"):
        api.Predictor.regression(model, _Pair(), Y[:5], idx0, 2, (1.0, 0.1), 1e-3)
    with pytest.raises(ValueError, match="one noise variance per training row"):
        api.Predictor.regression(model, _Pair(), Y, idx0, 2, (1.0, 0.1, 0.2), 1e-3, noisepar="different")
    with pytest.raises(api.FlgpError, match="noisepar"):
        api.Predictor.regression(model, _Pair(), Y, idx0, 2, (1.0, 0.1), 1e-3, noisepar="other")
    with pytest.raises(ValueError, match="one entry per value of t"):
        api.Predictor.logit(model, _Pair(), idx0, 2, [1.0, 2.0], Y, col=[0])
    with pytest.raises(ValueError, match="one row per entry of idx0"):
        api.Predictor.logit(model, _Pair(), idx0, 2, [1.0, 2.0], Y[:4])
    model.free()
    with pytest.raises(ValueError, match="freed"):
        api.Predictor.regression(model, _Pair(), Y, idx0, 2, (1.0, 0.1), 1e-3)
