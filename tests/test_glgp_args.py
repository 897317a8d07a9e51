"""CPU: the GLGP bandwidth-grid entries (include/flgp_hip.h) are declared, exported and bound, and both the
library and the Python wrapper refuse bad arguments before any device work, so these run without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from flgp_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("flgp_glgp_neighbours", "flgp_glgp_spectrum_grid", "flgp_dev_glgp_spectrum_grid", "flgp_dev_glgp_select",
         "flgp_dev_glgp_similarity", "flgp_dev_glgp_distances", "flgp_glgp_last_iterations")


def _refused(rc, what):
    assert rc == -1, rc
    msg = _lib.lib().flgp_last_error().decode()
    assert what in msg, msg
    return msg


def test_glgp_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flgp_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(L, name), name
        assert name in _lib.declared_symbols(), name
    _lib.lib()
    assert callable(api.glgp_spectrum_grid) and callable(api.glgp_neighbours)
    assert int(re.search(r"#define\s+FLGP_RMAX\s+(\d+)", text).group(1)) == 32       # the k-NN's limit is not this route's


def _host(X=True, n=10, d=3, K=4, a2=(0.5, 2.0), l=None, sparse=1, thr=0.3, values=True, vectors=False, pairs=None):
    L = _lib.lib()
    Xa = np.asfortranarray(np.arange(30.0).reshape(10, 3)); a2a = np.array(a2, dtype=np.float64) if a2 is not None else None
    v = np.zeros(64); V = np.zeros(4096)
    return L.flgp_glgp_spectrum_grid(Xa.ctypes.data if X else None, n, d, K, a2a.ctypes.data if a2a is not None else None,
                                     len(a2) if l is None else l, sparse, thr, 1, v.ctypes.data if values else None,
                                     V.ctypes.data if vectors else None, pairs, None, None)


def test_library_refuses_before_any_device_work():
    for msg in (_refused(_host(X=False), "null pointer"), _refused(_host(a2=None, l=1), "null pointer"),
                _refused(_host(values=False), "all NULL"), _refused(_host(n=2, K=1), "n=2"),
                _refused(_host(n=32769), "n=32769"), _refused(_host(d=0), "1 <= d"), _refused(_host(d=16385), "1 <= d"),
                _refused(_host(K=0), "K=0"), _refused(_host(K=11), "K=11"), _refused(_host(l=0), "at least one bandwidth"),
                _refused(_host(a2=(0.5, -1.0)), "bandwidth 1 (a2=-1): "), _refused(_host(a2=(float("inf"),)), "bandwidth 0 (a2=inf): "),
                _refused(_host(a2=(float("nan"),)), "bandwidth 0 (a2=nan): "),
                _refused(_host(thr=0.0), "threshold"), _refused(_host(thr=-0.1), "threshold"),
                _refused(_host(thr=float("nan")), "threshold"), _refused(_host(thr=float("inf")), "threshold"),
                _refused(_host(thr=1.06), "neighbours")):
        assert "glgp" in msg, msg
    # the dense route ignores the threshold: with a bad one, the next refusal in line is reached
    _refused(_host(sparse=0, thr=float("nan"), K=0), "K=0")
    # r = n is allowed (thr n + 0.5 rounds to n): the refusal that follows is another one
    _refused(_host(thr=1.04, K=11), "K=11")


def test_handles_are_cleared_on_refusal():
    out = (ctypes.c_void_p * 2)(1, 1)
    _refused(_host(K=11, values=False, pairs=ctypes.addressof(out)), "K=11")
    assert out[0] is None and out[1] is None


def test_device_twin_and_stage_entries_refuse_before_any_device_work():
    L = _lib.lib()
    X = np.zeros((10, 3), order="F"); a2 = np.array([1.0, 0.0]); v = np.zeros(64); j = np.zeros(16, dtype=np.int32)
    x, a, o = X.ctypes.data, a2.ctypes.data, v.ctypes.data
    assert "glgp" in _refused(L.flgp_dev_glgp_spectrum_grid(None, None, 10, 10, 3, 4, a, 1, 1, 0.3, 1, o, None, None, None), "null pointer")
    _refused(L.flgp_dev_glgp_spectrum_grid(None, x, 10, 10, 3, 4, a, 1, 1, 0.3, 1, None, None, None, None), "all NULL")
    _refused(L.flgp_dev_glgp_spectrum_grid(None, x, 10, 10, 3, 4, a, 2, 1, 0.3, 1, o, None, None, None), "bandwidth 1 (a2=0): ")
    _refused(L.flgp_dev_glgp_spectrum_grid(None, x, 10, 9, 3, 4, a, 1, 1, 0.3, 1, o, None, None, None), "leading dimension")
    _refused(L.flgp_dev_glgp_spectrum_grid(None, x, 10, 10, 3, 4, a, 1, 1, 2.0, 1, o, None, None, None), "neighbours")
    _refused(L.flgp_dev_glgp_select(None, None, 4, 4, 3, o, j.ctypes.data, o), "null pointer")
    _refused(L.flgp_dev_glgp_select(None, x, 4, 3, 3, o, j.ctypes.data, o), "ldd")
    _refused(L.flgp_dev_glgp_select(None, x, 4, 4, 5, o, j.ctypes.data, o), "r=5")
    _refused(L.flgp_dev_glgp_select(None, x, 4, 4, 0, o, j.ctypes.data, o), "r=0")
    _refused(L.flgp_dev_glgp_similarity(None, x, 4, 4, None, j.ctypes.data, 1.0, o, 4, None), "null pointer")
    _refused(L.flgp_dev_glgp_similarity(None, x, 4, 4, o, j.ctypes.data, 1.0, o, 3, None), "ldz=3")


def test_wrapper_refuses_before_any_device_work():
    X = np.arange(24.0).reshape(8, 3); Xn = np.arange(6.0).reshape(2, 3)
    for kw in (dict(K=0), dict(K=11), dict(K=None), dict(K=3, a2s=()), dict(K=3, threshold=0.0), dict(K=3, threshold=-1.0),
               dict(K=3, threshold=float("nan")), dict(K=3, threshold=float("inf")), dict(K=3, threshold=1.06)):
        with pytest.raises(ValueError):
            api.glgp_spectrum_grid(X, Xn, **kw)
    with pytest.raises(ValueError, match="columns"):
        api.glgp_spectrum_grid(X, np.zeros((2, 4)), 3)
    with pytest.raises(ValueError, match="at least 3 rows"):
        api.glgp_spectrum_grid(X[:1], Xn[:1], 1)
    # what the wrapper leaves to the library is refused there, still without a device
    with pytest.raises(api.FlgpError, match=r"bandwidth 1 \(a2=-2\): glgp"):
        api.glgp_spectrum_grid(X, Xn, 3, a2s=(1.0, -2.0))
    with pytest.raises(api.FlgpError, match=r"bandwidth 0 \(a2=-2\): glgp"):
        api.glgp_spectrum_grid(X, Xn, 3, a2s=(-2.0,), resident=True, sparse=False, threshold=float("nan"))
    assert api.glgp_neighbours(0.01, 2100) == 21 and api.glgp_neighbours(0.001, 100) == 3
