"""CPU: the entries of the greedy design (include/flgp_hip.h) are declared, exported and bound, and every
refusal made before a handle is read arrives with FLGP_ERR_INVALID, the name predictor_design and the documented order; so
these run without a GPU.  What reads a live handle -- its kind, a Nystrom handle, per-row noise at create, the device, the noise,
the values of X -- is in tests/test_gpu_predictor_design.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import predictor_design_cases as dc
from flgp_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("flgp_dev_predictor_design_workspace", "flgp_dev_predictor_design_rows", "flgp_predictor_design", "flgp_dev_predictor_design")
FAKE = 8               # a non-null pointer: every refusal here comes before it is looked at


def _message():
    return _lib.lib().flgp_last_error().decode()


def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flgp_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(L, name), name
        assert name in _lib.declared_symbols(), name
    assert callable(api.Predictor.design)


def _design(h=None, X=FAKE, n=4, B=2, noise=None, picks=FAKE):
    return _lib.lib().flgp_predictor_design(h, X, n, B, noise, picks, None, None)


def _dev_design(h=None, X=FAKE, n=4, ldx=4, B=2, noise=None, picks=FAKE):
    return _lib.lib().flgp_dev_predictor_design(None, h, X, n, ldx, B, noise, picks, None, None)


@pytest.mark.parametrize("call", [_design, _dev_design])
def test_design_refuses_in_order_without_a_handle(call):
    # 1: null picks, whatever else is wrong
    assert call(picks=None, X=None, n=0) == -1 and _message() == "predictor_design: null pointer (picks)"
    assert call(picks=None, h=FAKE) == -1 and _message() == "predictor_design: null pointer (picks)"
    # 2: a null h comes before the rows and the shapes
    for kw in (dict(), dict(X=None), dict(n=0), dict(B=0), dict(B=5)):
        assert call(**kw) == -1 and _message() == "predictor_design: null handle", (kw, _message())


@pytest.mark.parametrize("call", [_design, _dev_design])
def test_design_refuses_the_rows_and_shapes_before_the_handle_is_read(call):
    """refusal 3 with a handle that is never dereferenced"""
    chain = [(dict(X=None), "null pointer"), (dict(n=0), "need n >= 1 (n=0)"), (dict(n=-2), "need n >= 1 (n=-2)"),
             (dict(B=0), "need 1 <= B <= n (B=0, n=4)"), (dict(B=-1), "need 1 <= B <= n (B=-1, n=4)"),
             (dict(B=5), "need 1 <= B <= n (B=5, n=4)")]
    for kw, text in chain:
        assert call(h=FAKE, **kw) == -1 and _message() == "predictor_design: " + text, (kw, _message())
    # in order: the pointer, then n, then B
    assert call(h=FAKE, X=None, n=0, B=0) == -1 and _message() == "predictor_design: null pointer"
    assert call(h=FAKE, n=0, B=0) == -1 and _message() == "predictor_design: need n >= 1 (n=0)"


def test_the_device_entry_refuses_a_short_leading_dimension():
    assert _dev_design(h=FAKE, ldx=3) == -1 and _message() == "predictor_design: a leading dimension is below n = 4"
    assert _dev_design(h=FAKE, ldx=3, B=5) == -1 and _message() == "predictor_design: need 1 <= B <= n (B=5, n=4)"


def _rows(idx=FAKE, val=FAKE, n=4, r=2, P=FAKE, ldp=16, s=5, K=3, d=0.1, B=2, picks=FAKE, work=FAKE, bytes_=None):
    if bytes_ is None:
        bytes_ = dc.workspace_bytes(n, r, s, K, B) if dc.shape_ok(n, r, s, K, B) else 1 << 20
    return _lib.lib().flgp_dev_predictor_design_rows(None, idx, val, n, r, P, ldp, s, K, d, B, picks, None, None, work, bytes_)


ROWS_REFUSALS = [
    (dict(idx=None), "null pointer"), (dict(val=None), "null pointer"), (dict(P=None), "null pointer"), (dict(picks=None), "null pointer"),
    (dict(work=None), "null pointer"),
    (dict(n=0), "bad shape (n=0, r=2, s=5, K=3, B=2)"), (dict(r=0), "bad shape"), (dict(r=33), "bad shape"), (dict(s=0), "bad shape"),
    (dict(s=32769), "bad shape"), (dict(K=0), "bad shape"), (dict(B=0), "bad shape"), (dict(B=5), "bad shape (n=4, r=2, s=5, K=3, B=5)"),
    (dict(ldp=2), "ldp=2 is below K = 3"),
    (dict(d=0.0), "the observation variance d = 0 must be finite and positive"), (dict(d=-1.0), "must be finite and positive"),
    (dict(d=float("nan")), "must be finite and positive"), (dict(d=float("inf")), "must be finite and positive"),
    (dict(bytes_=dc.workspace_bytes(4, 2, 5, 3, 2) - 1), f"the workspace holds {dc.workspace_bytes(4, 2, 5, 3, 2) - 1} bytes, "
                                                          f"{dc.workspace_bytes(4, 2, 5, 3, 2)} are needed"),
]


@pytest.mark.parametrize("kw,text", ROWS_REFUSALS)
def test_rows_refuses_before_any_launch(kw, text):
    assert _rows(**kw) == -1
    assert _message().startswith("predictor_design_rows: ") and text in _message(), _message()


def test_the_workspace_query():
    L = _lib.lib()
    for case in dc.CASES + [(100000, 10, 5000, 200, 1000), (1000000, 10, 5000, 200, 10), (5, 32, 32768, 7, 5)]:
        assert L.flgp_dev_predictor_design_workspace(*case) == dc.workspace_bytes(*case), case
    for bad in ((0, 2, 5, 3, 1), (4, 0, 5, 3, 2), (4, 33, 5, 3, 2), (4, 2, 0, 3, 2), (4, 2, 32769, 3, 2), (4, 2, 5, 0, 2), (4, 2, 5, 3, 0),
                (4, 2, 5, 3, 5), (-1, 2, 5, 3, 1)):
        assert L.flgp_dev_predictor_design_workspace(*bad) == 0, bad


def test_python_checks_its_arrays_before_the_library():
    p = api.Predictor.__new__(api.Predictor)
    p._h = ctypes.c_void_p(FAKE)                               # never dereferenced
    p._model = api.SpectrumModel(ctypes.c_void_p(0), dims=(100, 3, 10, 3, 4, 0, 2, 1))
    p.d, p.s, p.r, p.K, p.groups, p.q, p.kind, p.ldp, p.iters, p.draw_shape = 3, 10, 3, 4, 1, 2, "regression", 16, None, None
    X = np.zeros((4, 3))
    with pytest.raises(ValueError, match="X has 5 columns"):
        p.design(np.zeros((4, 5)), 2)
    with pytest.raises(ValueError, match="at least one row"):
        p.design(np.zeros((0, 3)), 1)
    for B in (0, 5, -1):
        with pytest.raises(ValueError, match="B must be between 1 and the 4 rows of X"):
            p.design(X, B)
    with pytest.raises(ValueError, match="noise must be None or one variance"):
        p.design(X, 2, noise=np.ones(4))
    p._h = None
    with pytest.raises(ValueError, match="freed"):
        p.design(X, 2)
