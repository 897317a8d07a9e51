"""CPU: the entries of the predictor's update (include/flgp_hip.h) are declared, exported and bound, and every
refusal made before a handle is read arrives with FLGP_ERR_INVALID, the name predictor_update and the documented order, *out
cleared; so these run without a GPU.  What reads a live handle -- its kind, a Nystrom handle, per-row noise at create, the
values of Y and the noise -- is in tests/test_gpu_predictor_update.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from flgp_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("flgp_dev_predictor_gram_workspace", "flgp_dev_predictor_gram", "flgp_predictor_update", "flgp_dev_predictor_update")
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
    assert callable(api.Predictor.update)


def _update(h=None, X=FAKE, n=4, Y=FAKE, noise=None, n_noise=0, out=True):
    o = ctypes.c_void_p(1)
    rc = _lib.lib().flgp_predictor_update(h, X, n, Y, noise, n_noise, ctypes.byref(o) if out else None)
    return rc, o.value


def _dev_update(h=None, X=FAKE, n=4, ldx=4, Y=FAKE, ldy=4, noise=None, n_noise=0, out=True):
    o = ctypes.c_void_p(1)
    rc = _lib.lib().flgp_dev_predictor_update(None, h, X, n, ldx, Y, ldy, noise, n_noise, ctypes.byref(o) if out else None)
    return rc, o.value


@pytest.mark.parametrize("call", [_update, _dev_update])
def test_update_refuses_in_order_without_a_handle(call):
    # 1: a null out, whatever else is wrong
    assert call(out=False, X=None, n=0)[0] == -1 and _message() == "predictor_update: null pointer (out)"
    # 2: a null h comes before the arrays and the shapes, and *out is cleared
    for kw in (dict(), dict(X=None), dict(Y=None), dict(n=0), dict(noise=FAKE, n_noise=3), dict(n_noise=1)):
        rc, o = call(**kw)
        assert rc == -1 and o is None and _message() == "predictor_update: null handle", (kw, _message())


@pytest.mark.parametrize("call", [_update, _dev_update])
def test_update_refuses_the_arrays_and_shapes_before_the_handle_is_read(call):
    """refusal 3 with a handle that is never dereferenced"""
    h = FAKE
    chain = [(dict(X=None), "null pointer"), (dict(Y=None), "null pointer"), (dict(n=0), "need n_b >= 1 (n_b=0)"),
             (dict(n=-2), "need n_b >= 1 (n_b=-2)"),
             (dict(n_noise=1), "n_noise=1 must be 0 with a NULL noise, 1 or n_b=4"),
             (dict(noise=FAKE, n_noise=0), "n_noise=0 must be 0 with a NULL noise, 1 or n_b=4"),
             (dict(noise=FAKE, n_noise=3), "n_noise=3 must be 0 with a NULL noise, 1 or n_b=4")]
    for kw, text in chain:
        rc, o = call(h=h, **kw)
        assert rc == -1 and o is None and _message() == "predictor_update: " + text, (kw, _message())
    # in order: the pointers, then n_b, then the noise length
    rc, o = call(h=h, X=None, n=0, noise=FAKE, n_noise=3)
    assert rc == -1 and _message() == "predictor_update: null pointer"
    rc, o = call(h=h, n=0, noise=FAKE, n_noise=3)
    assert rc == -1 and _message() == "predictor_update: need n_b >= 1 (n_b=0)"


def test_the_device_entry_refuses_short_leading_dimensions():
    for kw in (dict(ldx=3), dict(ldy=3)):
        rc, o = _dev_update(h=FAKE, **kw)
        assert rc == -1 and o is None and _message() == "predictor_update: a leading dimension is below n_b = 4"


def _gram(idx=FAKE, val=FAKE, n=4, r=2, P=FAKE, ldp=16, s=5, K=3, q=2, w=FAKE, Y=FAKE, ldy=4, S=FAKE, lds=5, work=FAKE, bytes_=None):
    L = _lib.lib()
    if bytes_ is None:
        bytes_ = 8 * 25 * ((n + 255) // 256 if n > 0 else 1)
    return L.flgp_dev_predictor_gram(None, idx, val, n, r, P, ldp, s, K, q, w, Y, ldy, S, lds, work, bytes_)


GRAM_REFUSALS = [
    (dict(idx=None), "null pointer"), (dict(val=None), "null pointer"), (dict(P=None), "null pointer"), (dict(w=None), "null pointer"),
    (dict(S=None), "null pointer"), (dict(work=None), "null pointer"), (dict(Y=None), "null pointer (q = 2 needs Y)"),
    (dict(n=0), "bad shape (n=0, r=2, s=5, K=3, q=2)"), (dict(r=0), "bad shape"), (dict(r=33), "bad shape"), (dict(s=0), "bad shape"),
    (dict(K=0), "bad shape"), (dict(q=-1), "bad shape"),
    (dict(K=23105, q=0, Y=None, ldp=1 << 20, lds=1 << 20), "K + q = 23105 is above 23104 columns"),
    (dict(ldp=4), "ldp=4 is below K + q = 5"), (dict(ldy=3), "ldy=3 is below n = 4"), (dict(lds=4), "lds=4 is below K + q = 5"),
    (dict(bytes_=199), "the workspace holds 199 bytes, 200 are needed"),
    (dict(n=257, ldy=257, bytes_=399), "the workspace holds 399 bytes, 400 are needed"),
]


@pytest.mark.parametrize("kw,text", GRAM_REFUSALS)
def test_gram_refuses_before_any_launch(kw, text):
    assert _gram(**kw) == -1
    assert _message().startswith("predictor_gram: ") and text in _message(), _message()


def test_gram_refuses_in_order():
    chain = [dict(idx=None), dict(n=0), dict(ldp=4), dict(ldy=3), dict(lds=4), dict(bytes_=0)]
    texts = ["null pointer", "bad shape (n=0, r=2, s=5, K=3, q=2)", "ldp=4 is below K + q = 5", "ldy=3 is below n = 4",
             "lds=4 is below K + q = 5", "the workspace holds 0 bytes, 200 are needed"]
    for at in range(len(chain)):
        kw = {}
        for later in reversed(chain[at:]):
            kw.update(later)
        if at >= 2:
            kw.pop("n", None)
        assert _gram(**kw) == -1 and _message() == "predictor_gram: " + texts[at], (at, _message())


def test_gram_workspace():
    L = _lib.lib()
    assert L.flgp_dev_predictor_gram_workspace(1, 3, 2) == 8 * 25
    assert L.flgp_dev_predictor_gram_workspace(256, 200, 1) == 8 * 201 * 201
    assert L.flgp_dev_predictor_gram_workspace(257, 200, 1) == 2 * 8 * 201 * 201
    assert L.flgp_dev_predictor_gram_workspace(100000, 200, 0) == 64 * 8 * 200 * 200          # no more chunks than one launch takes
    assert L.flgp_dev_predictor_gram_workspace(100000, 2000, 1) == 8 * 8 * 2001 * 2001        # nor more than 256 MiB
    import predictor_update_cases as uc
    for n, K, q in ((1, 3, 2), (5000, 64, 1), (100000, 200, 1), (1 << 20, 2000, 3)):
        assert L.flgp_dev_predictor_gram_workspace(n, K, q) == uc.workspace_bytes(n, K, q)
    for bad in ((0, 3, 2), (4, 0, 2), (4, 3, -1)):
        assert L.flgp_dev_predictor_gram_workspace(*bad) == 0


def test_python_checks_its_arrays_before_the_library():
    p = api.Predictor.__new__(api.Predictor)
    p._h = ctypes.c_void_p(FAKE)                               # never dereferenced
    p._model = api.SpectrumModel(ctypes.c_void_p(0), dims=(100, 3, 10, 3, 4, 0, 2, 1))
    p.d, p.s, p.r, p.K, p.groups, p.q, p.kind, p.ldp, p.iters, p.draw_shape = 3, 10, 3, 4, 1, 2, "regression", 16, None, None
    X = np.zeros((4, 3))
    with pytest.raises(ValueError, match="X has 5 columns"):
        p.update(np.zeros((4, 5)), np.zeros((4, 2)))
    with pytest.raises(ValueError, match="at least one row"):
        p.update(np.zeros((0, 3)), np.zeros((0, 2)))
    for Y in (np.zeros((3, 2)), np.zeros((4, 1)), np.zeros(4), np.zeros((4, 2, 1))):
        with pytest.raises(ValueError, match="Y must have one row per row of X and q = 2 columns"):
            p.update(X, Y)
    with pytest.raises(api.FlgpError, match="predictor_update: n_noise=3 must be 0 with a NULL noise, 1 or n_b=4"):
        p.update(X, np.zeros((4, 2)), noise=np.ones(3))
    p._h = None
    with pytest.raises(ValueError, match="freed"):
        p.update(X, np.zeros((4, 2)))
