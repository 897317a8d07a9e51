"""CPU: the entries of the joint posterior of served rows (include/flgp_hip.h) are declared, exported and bound,
and every refusal made before a handle is read arrives with FLGP_ERR_INVALID and the documented name, *out cleared; so these
run without a GPU.  What reads a live handle -- its kind, S, the column count, g, `var` on a draws handle -- is in
tests/test_gpu_predictor_draws.py and tests/test_gpu_predictor_covariance.py.  The Python class checks its arrays, and the kind
of its handle, before it touches the library."""
import ctypes
import os
import re

import numpy as np
import pytest

from flgp_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("flgp_dev_predictor_cols", "flgp_dev_predictor_draws_fold", "flgp_predictor_draws_create", "flgp_predictor_draws_normals",
         "flgp_predictor_features", "flgp_dev_predictor_features", "flgp_predictor_covariance")
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
    assert re.search(r"#define\s+FLGP_PREDICTOR_DRAWS\s+3\b", text)
    for method in ("draws", "normals", "features", "covariance"):
        assert callable(getattr(api.Predictor, method))
    assert api.Predictor._KIND[3] == "draws"


def test_draws_create_refuses_before_any_device_work():
    L = _lib.lib()
    assert L.flgp_predictor_draws_create(None, 0, 1, None) == -1 and _message() == "predictor_draws: null pointer"
    out = ctypes.c_void_p(1)
    assert L.flgp_predictor_draws_create(None, 0, 1, ctypes.byref(out)) == -1 and _message() == "predictor_draws: null handle"
    assert out.value is None                                   # *out is cleared, and the null handle comes before S
    xi = np.zeros(4)
    assert L.flgp_predictor_draws_normals(None, None) == -1 and _message() == "predictor_draws_normals: null pointer"
    assert L.flgp_predictor_draws_normals(None, xi.ctypes.data) == -1 and _message() == "predictor_draws_normals: null handle"


def _cols(idx=FAKE, val=FAKE, n=4, r=2, P=FAKE, ldp=16, s=5, c0=0, nc=3, out=FAKE, ldo=4):
    return _lib.lib().flgp_dev_predictor_cols(None, idx, val, n, r, P, ldp, s, c0, nc, out, ldo)


COLS_REFUSALS = [
    (dict(idx=None), "null pointer"), (dict(val=None), "null pointer"), (dict(P=None), "null pointer"), (dict(out=None), "null pointer"),
    (dict(n=0), "bad shape (n=0, r=2, s=5, nc=3)"), (dict(r=0), "bad shape"), (dict(r=33), "bad shape"), (dict(s=0), "bad shape"),
    (dict(nc=0), "bad shape (n=4, r=2, s=5, nc=0)"),
    (dict(c0=-1), "columns [-1, 2) are outside ldp = 16"), (dict(c0=14), "columns [14, 17) are outside ldp = 16"),
    (dict(nc=17), "columns [0, 17) are outside ldp = 16"), (dict(ldp=2), "columns [0, 3) are outside ldp = 2"),
    (dict(ldo=3), "ldo=3 is below n = 4"),
]


@pytest.mark.parametrize("kw,text", COLS_REFUSALS)
def test_cols_refuses_before_any_launch(kw, text):
    assert _cols(**kw) == -1
    assert _message().startswith("predictor_cols: ") and text in _message(), _message()


def test_cols_refuses_in_order():
    chain = [dict(idx=None), dict(n=0), dict(c0=-1), dict(ldo=-1)]
    texts = ["null pointer", "bad shape (n=0, r=2, s=5, nc=3)", "columns [-1, 2) are outside ldp = 16", "ldo=-1 is below n = 4"]
    for at in range(len(chain)):
        kw = {}
        for later in reversed(chain[at:]):
            kw.update(later)
        assert _cols(**kw) == -1 and _message() == "predictor_cols: " + texts[at], (at, _message())


def _fold(P=FAKE, ldp=16, s=5, groups=2, K=3, q=2, S=4, xi=FAKE, Pd=FAKE, ldd=16):
    return _lib.lib().flgp_dev_predictor_draws_fold(None, P, ldp, s, groups, K, q, S, 7, xi, Pd, ldd)


FOLD_REFUSALS = [
    (dict(P=None), "null pointer"), (dict(xi=None), "null pointer"), (dict(Pd=None), "null pointer"),
    (dict(s=0), "bad shape (s=0, groups=2, K=3, q=2, S=4)"), (dict(groups=0), "bad shape"), (dict(K=0), "bad shape"),
    (dict(q=0), "bad shape"), (dict(S=0), "bad shape"),
    (dict(groups=1 << 15, q=1 << 10, S=1 << 10), "groups q S = 34359738368 columns overflow an int"),
    (dict(groups=1, q=1, S=2 ** 31 - 15), "columns overflow an int"),
    (dict(ldp=9), "ldp=9 is below groups (K + q) = 10"), (dict(ldd=15), "ldd=15 is below groups q S = 16"),
]


@pytest.mark.parametrize("kw,text", FOLD_REFUSALS)
def test_fold_refuses_before_any_launch(kw, text):
    assert _fold(**kw) == -1
    assert _message().startswith("predictor_draws_fold: ") and text in _message(), _message()


def test_features_and_covariance_refuse_before_the_handle_is_read():
    L = _lib.lib()
    X = np.zeros((5, 3), order="F"); Z = np.zeros((5, 4), order="F")
    x, z = X.ctypes.data, Z.ctypes.data
    for args, text in (((None, 0, None, 5, z), "null pointer"), ((None, 0, x, 5, None), "null pointer"),
                       ((None, 0, x, 0, z), "need n >= 1 (n=0)"), ((None, 0, x, 5, z), "null handle")):
        assert L.flgp_predictor_features(*args) == -1 and _message() == "predictor_features: " + text, _message()
    for args, text in (((None, None, 0, None, 5, 5, z, 5), "null pointer"), ((None, None, 0, x, 5, 5, None, 5), "null pointer"),
                       ((None, None, 0, x, 0, 5, z, 5), "need n >= 1 (n=0)"),
                       ((None, None, 0, x, 5, 4, z, 5), "a leading dimension is below n = 5"),
                       ((None, None, 0, x, 5, 5, z, 4), "a leading dimension is below n = 5"),
                       ((None, None, -1, x, 5, 5, z, 5), "null handle")):           # g is read against the handle's groups
        assert L.flgp_dev_predictor_features(*args) == -1 and _message() == "predictor_features: " + text, _message()
    for args, text in (((None, 0, None, 5, None, 0, z), "null pointer"), ((None, 0, x, 5, None, 0, None), "null pointer"),
                       ((None, 0, x, 0, None, 0, z), "need na >= 1 and nb >= 1 (na=0, nb=0)"),
                       ((None, 0, x, 5, x, 0, z), "need na >= 1 and nb >= 1 (na=5, nb=0)"),
                       ((None, 0, x, 5, None, 0, z), "null handle"),                # nb is not looked at without Xb
                       ((None, 0, x, 5, x, 5, z), "null handle")):
        assert L.flgp_predictor_covariance(*args) == -1 and _message() == "predictor_covariance: " + text, _message()


def _handle_of_kind(kind, groups=1, q=1):
    """a Predictor that never was the library's: what the methods check before they call it"""
    p = api.Predictor.__new__(api.Predictor)
    p._h = ctypes.c_void_p(FAKE)                               # never dereferenced
    p._model = api.SpectrumModel(ctypes.c_void_p(0), dims=(100, 3, 10, 3, 4, 0, 2, 1))
    p.d, p.s, p.r, p.K, p.groups, p.q, p.kind, p.ldp, p.iters, p.draw_shape = 3, 10, 3, 4, groups, q, kind, 16, None, None
    return p


@pytest.mark.parametrize("kind", ["pg", "draws"])
def test_python_refuses_a_handle_without_a_covariance_operand(kind):
    p = _handle_of_kind(kind)
    X = np.zeros((4, 3))
    for call, who in ((lambda: p.draws(3, 1), "predictor_draws"), (lambda: p.features(X), "predictor_features"),
                      (lambda: p.covariance(X), "predictor_covariance")):
        with pytest.raises(api.FlgpError, match=f"{who}: a handle of kind {api.Predictor._KIND.index(kind)} has no covariance operand"):
            call()
    p._h = None


def test_python_checks_its_arguments_before_the_library():
    p = _handle_of_kind("logit", groups=3)
    X = np.zeros((4, 3))
    with pytest.raises(ValueError, match="S must be at least 1"):
        p.draws(0, 1)
    with pytest.raises(ValueError, match="overflows an int"):
        p.draws(2 ** 30, 1)
    for g in (-1, 3):
        with pytest.raises(IndexError, match=f"group {g} outside 0..2"):
            p.features(X, group=g)
        with pytest.raises(IndexError, match=f"group {g} outside 0..2"):
            p.covariance(X, group=g)
    with pytest.raises(ValueError, match="columns"):
        p.features(np.zeros((4, 4)))
    with pytest.raises(ValueError, match="at least one row"):
        p.features(np.zeros((0, 3)))
    with pytest.raises(ValueError, match="Xa has 4 columns"):
        p.covariance(np.zeros((4, 4)))
    with pytest.raises(ValueError, match="Xb has 2 columns"):
        p.covariance(X, np.zeros((4, 2)))
    with pytest.raises(ValueError, match="Xb must have at least one row"):
        p.covariance(X, np.zeros((0, 3)))
    with pytest.raises(ValueError, match="diag_term needs Xb=None"):
        p.covariance(X, X, diag_term=True)
    with pytest.raises(api.FlgpError, match="predictor_draws_normals: the handle is not a draws one"):
        p.normals()
    p._h = None
    for call in (lambda: p.draws(3, 1), lambda: p.features(X), lambda: p.covariance(X), lambda: p.normals()):
        with pytest.raises(ValueError, match="freed"):
            call()
