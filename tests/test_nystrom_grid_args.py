"""CPU: the Nystrom bandwidth-grid entries (include/flgp_hip.h) are declared, exported and bound, and both
the library and the Python wrappers refuse bad arguments before any device work, so these run without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from flgp_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("flgp_nystrom_grid_create", "flgp_nystrom_grid_dims", "flgp_nystrom_grid_values", "flgp_nystrom_grid_free",
         "flgp_nystrom_grid_extend", "flgp_nystrom_grid_extend_resident", "flgp_nystrom_grid_extend_all",
         "flgp_nystrom_grid_extend_all_resident", "flgp_dev_nystrom_grid_create", "flgp_dev_nystrom_grid_extend",
         "flgp_dev_nystrom_grid_extend_all")


def _refused(rc, what):
    assert rc == -1, rc
    assert what in _lib.lib().flgp_last_error().decode()


def test_grid_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flgp_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(L, name), name
        assert name in _lib.declared_symbols(), name
    _lib.lib()
    assert callable(api.nystrom_spectrum_grid) and callable(api.NystromGrid.extend_all)
    assert int(re.search(r"#define\s+FLGP_NYSTROM_GRID_BATCH\s+(\d+)", text).group(1)) >= 2


def test_library_refuses_before_any_device_work():
    L = _lib.lib()
    U = np.asfortranarray(np.arange(30.0).reshape(10, 3)); a2 = np.array([0.5, -1.0, 2.0])
    h = ctypes.c_void_p(1)
    _refused(L.flgp_nystrom_grid_create(None, 10, 3, a2.ctypes.data, 3, 4, 1, ctypes.byref(h)), "null pointer")
    assert h.value is None                                     # the handle is cleared on every refusal
    _refused(L.flgp_nystrom_grid_create(U.ctypes.data, 10, 3, None, 3, 4, 1, ctypes.byref(h)), "null pointer")
    _refused(L.flgp_nystrom_grid_create(U.ctypes.data, 10, 3, a2.ctypes.data, 3, 4, 1, None), "null pointer")
    _refused(L.flgp_nystrom_grid_create(U.ctypes.data, 10, 3, a2.ctypes.data, 0, 4, 1, ctypes.byref(h)), "at least one bandwidth")
    _refused(L.flgp_nystrom_grid_create(U.ctypes.data, 10, 3, a2.ctypes.data, 3, 11, 1, ctypes.byref(h)), "K=11")
    _refused(L.flgp_nystrom_grid_create(U.ctypes.data, 10, 3, a2.ctypes.data, 3, 0, 1, ctypes.byref(h)), "K=0")
    _refused(L.flgp_nystrom_grid_create(U.ctypes.data, 1, 3, a2.ctypes.data, 3, 1, 1, ctypes.byref(h)), "s=1")
    # the device twin checks the bandwidths before it touches the device: the SE grid's message
    _refused(L.flgp_dev_nystrom_grid_create(None, U.ctypes.data, 10, 10, 3, a2.ctypes.data, 3, 4, 1, ctypes.byref(h)),
             "bandwidth 1 (a2=-1): ")
    _refused(L.flgp_dev_nystrom_grid_create(None, U.ctypes.data, 10, 9, 3, a2.ctypes.data, 1, 4, 1, ctypes.byref(h)), "leading dimension")
    _refused(L.flgp_dev_nystrom_grid_create(None, U.ctypes.data, 10, 10, 0, a2.ctypes.data, 1, 4, 1, ctypes.byref(h)), "1 <= d")
    # a null handle
    _refused(L.flgp_nystrom_grid_dims(None, None, None, None, None, None), "null handle")
    _refused(L.flgp_nystrom_grid_values(None, None, None), "null handle")
    v = np.zeros(8)
    _refused(L.flgp_nystrom_grid_extend(None, 0, U.ctypes.data, 10, None, v.ctypes.data), "null pointer")
    _refused(L.flgp_nystrom_grid_extend_resident(None, 0, U.ctypes.data, 10, ctypes.byref(h)), "null handle")
    _refused(L.flgp_nystrom_grid_extend_all(None, U.ctypes.data, 10, v.ctypes.data), "null pointer")
    _refused(L.flgp_nystrom_grid_extend_all_resident(None, U.ctypes.data, 10, ctypes.byref(h)), "null pointer")
    L.flgp_nystrom_grid_free(None)                             # like free(NULL)


def test_constructor_checks():
    U = np.arange(30.0).reshape(10, 3)
    with pytest.raises(ValueError):
        api.nystrom_spectrum_grid(U, (1.0,), 11)               # K > s
    with pytest.raises(ValueError):
        api.nystrom_spectrum_grid(U, (1.0,), 0)
    with pytest.raises(ValueError):
        api.nystrom_spectrum_grid(U, (1.0,))                   # K is required
    with pytest.raises(ValueError):
        api.nystrom_spectrum_grid(U, (), 3)                    # l = 0
    with pytest.raises(ValueError):
        api.nystrom_spectrum_grid(np.zeros((2, 3, 4)), (1.0,), 1)


def _grid(l=3, s=10, d=3, K=4):
    """a wrapper around a null handle: every check below fails before the handle would be used"""
    return api.NystromGrid(ctypes.c_void_p(0), np.linspace(0.5, 1.5, l), s, d, K)


def test_wrapper_checks_columns_index_and_use_after_free():
    g = _grid()
    assert (g.s, g.d, g.l, g.K, g.workers) == (10, 3, 3, 4, 1)
    X = np.zeros((7, 3))
    for bad in (np.zeros((7, 2)), np.zeros((7, 4)), np.zeros(7)):
        with pytest.raises(ValueError, match="columns"):
            g.extend(0, bad)
        with pytest.raises(ValueError, match="columns"):
            g.extend_all(bad, resident=True)
    with pytest.raises(ValueError, match="at least one row"):
        g.extend_all(np.zeros((0, 3)))
    for i in (-1, 3, 100):
        with pytest.raises(IndexError, match="outside 0..2"):
            g.extend(i, X)
        with pytest.raises(IndexError):
            g.extend(i, X, resident=True)
    g.free()
    g.free()                                                   # twice is harmless
    for call in (lambda: g.extend(0, X), lambda: g.extend_all(X), lambda: g.values, lambda: g.distances_mean):
        with pytest.raises(ValueError, match="freed"):
            call()


def test_pipeline_stage_checks_need_no_device():
    """HipStages' grid stages check the owner's handle, the column count and the index before the library is called"""
    from flgp_amd.pipeline import HipStages
    st = object.__new__(HipStages)                             # no device behind it: only the checks are reached

    class T:                                                   # the shape is all the checks read
        def __init__(self, *shape):
            self.shape = shape
    with pytest.raises(ValueError, match="call nystrom_grid first"):
        st.nystrom_grid_extend(0, T(3, 5))
    st._nys_grids = {id(None): (ctypes.c_void_p(0), 3, 2, 4)}
    with pytest.raises(ValueError, match="columns"):
        st.nystrom_grid_extend_all(T(4, 5))
    with pytest.raises(IndexError):
        st.nystrom_grid_extend(2, T(3, 5))
    with pytest.raises(ValueError, match="call nystrom_grid first"):
        st.nystrom_grid_extend(0, T(3, 5), owner=st)           # another owner's grid is not this one's
