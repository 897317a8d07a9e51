"""CPU: the fitted-spectrum-model entries (include/flgp_hip.h) are declared, exported and bound; the
library and the Python wrappers refuse bad arguments before any device work, so these run without a GPU (the refusals
that need a live handle -- head rows, head K -- are in tests/test_gpu_spectrum_model.py); and the numpy restatement of the
extension (tests/np_spectrum_model.py) returns the fit rows of an oracle-only fit bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest

import np_spectrum_model as npm
from conftest import make_case
from flgp_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("flgp_heat_kernel_spectrum_model", "flgp_spectrum_model_dims", "flgp_spectrum_model_to_host",
         "flgp_spectrum_model_extend", "flgp_spectrum_model_extend_resident", "flgp_spectrum_model_free",
         "flgp_dev_spectrum_model_extend", "flgp_dev_extend_scale")


def _refused(rc, what):
    assert rc == -1, rc
    assert what in _lib.lib().flgp_last_error().decode()


def test_model_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flgp_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(L, name), name
        assert name in _lib.declared_symbols(), name
    _lib.lib()
    assert re.search(r"typedef\s+struct\s+flgp_spectrum_model\s+flgp_spectrum_model\s*;", text)
    assert callable(api.heat_kernel_spectrum_model) and callable(api.SpectrumModel.extend)


def test_library_refuses_before_any_device_work():
    L = _lib.lib()
    X = np.asfortranarray(np.arange(30.0).reshape(10, 3)); U = np.asfortranarray(X[:4])
    v = np.zeros(40); rows = np.zeros(4, dtype=np.int32)
    hm = ctypes.c_void_p(1); hp = ctypes.c_void_p(1); out = ctypes.c_void_p(1)

    def fit(kernel=b"lae", gl=b"rw", model=ctypes.byref(hm), pair=ctypes.byref(hp)):
        return L.flgp_heat_kernel_spectrum_model(X.ctypes.data, 10, 3, U.ctypes.data, 4, 3, 2, 2, kernel, gl, 0, 0.1, model, pair)
    _refused(fit(model=None), "null pointer")
    assert hp.value is None                                    # the handles are cleared on every refusal
    hp.value = 1
    assert fit(kernel=b"cosine") == -3 and b"kernel type is not supported" in L.flgp_last_error()
    assert hm.value is None and hp.value is None
    hm.value = 1; hp.value = 1
    assert fit(gl=b"sym") == -3
    assert hm.value is None and hp.value is None
    # the extension: pointers and counts first, then the handle
    _refused(L.flgp_spectrum_model_extend(None, None, 10, v.ctypes.data), "null pointer")
    _refused(L.flgp_spectrum_model_extend(None, X.ctypes.data, 10, None), "null pointer")
    _refused(L.flgp_spectrum_model_extend(None, X.ctypes.data, 0, v.ctypes.data), "n_new >= 1")
    _refused(L.flgp_spectrum_model_extend(None, X.ctypes.data, 10, v.ctypes.data), "null handle")
    _refused(L.flgp_spectrum_model_extend_resident(None, X.ctypes.data, 10, None, None, 0, None), "null pointer")
    _refused(L.flgp_spectrum_model_extend_resident(None, None, 10, None, None, 0, ctypes.byref(out)), "null pointer")
    assert out.value is None
    out.value = 1
    _refused(L.flgp_spectrum_model_extend_resident(None, X.ctypes.data, 0, None, None, 0, ctypes.byref(out)), "n_new >= 1")
    assert out.value is None
    out.value = 1
    _refused(L.flgp_spectrum_model_extend_resident(None, X.ctypes.data, -5, None, None, 0, ctypes.byref(out)), "n_new=-5")
    _refused(L.flgp_spectrum_model_extend_resident(None, X.ctypes.data, 10, None, rows.ctypes.data, -1, ctypes.byref(out)), "n_head >= 0")
    assert out.value is None
    out.value = 1
    _refused(L.flgp_spectrum_model_extend_resident(None, X.ctypes.data, 10, None, None, 0, ctypes.byref(out)), "null handle")
    assert out.value is None
    _refused(L.flgp_dev_spectrum_model_extend(None, None, None, 10, 10, v.ctypes.data, 10), "null pointer")
    _refused(L.flgp_dev_spectrum_model_extend(None, None, X.ctypes.data, 0, 10, v.ctypes.data, 10), "n_new >= 1")
    _refused(L.flgp_dev_spectrum_model_extend(None, None, X.ctypes.data, 10, 9, v.ctypes.data, 10), "leading dimension")
    _refused(L.flgp_dev_spectrum_model_extend(None, None, X.ctypes.data, 10, 10, v.ctypes.data, 9), "leading dimension")
    _refused(L.flgp_dev_spectrum_model_extend(None, None, X.ctypes.data, 10, 10, v.ctypes.data, 10), "null handle")
    _refused(L.flgp_spectrum_model_dims(None, None, None, None, None, None, None, None, None), "null handle")
    _refused(L.flgp_spectrum_model_to_host(None, None, None, None, None, None, None), "null handle")
    # the scaling stage
    _refused(L.flgp_dev_extend_scale(None, None, v.ctypes.data, 4, 2, None, None, v.ctypes.data), "extend_scale")
    _refused(L.flgp_dev_extend_scale(None, rows.ctypes.data, v.ctypes.data, 4, 2, None, None, None), "extend_scale")
    _refused(L.flgp_dev_extend_scale(None, rows.ctypes.data, v.ctypes.data, 4, 0, None, None, v.ctypes.data), "extend_scale")
    _refused(L.flgp_dev_extend_scale(None, rows.ctypes.data, v.ctypes.data, 4, 33, None, None, v.ctypes.data), "extend_scale")
    L.flgp_spectrum_model_free(None)                           # like free(NULL)


def _model(d=3, K=4):
    """a wrapper around a null handle: every check below fails before the handle would be used"""
    return api.SpectrumModel(ctypes.c_void_p(0), dims=(100, d, 10, 3, K, 0, 2, 1))


class _Pair:                                                   # what the wrapper's checks read of a resident pair
    def __init__(self, n, K, handle=ctypes.c_void_p(0)):
        self.n, self.K, self._h = n, K, handle


def test_wrapper_checks_and_use_after_free():
    m = _model()
    assert m.dims == {"n_fit": 100, "d": 3, "s": 10, "r": 3, "K": 4, "kernel": "lae", "gl": "cluster-normalized", "root": True}
    X = np.zeros((7, 3))
    for bad in (np.zeros((7, 2)), np.zeros((7, 4)), np.zeros(7)):
        with pytest.raises(ValueError, match="columns"):
            m.extend(bad)
        with pytest.raises(ValueError, match="columns"):
            m.extend(bad, resident=True)
    with pytest.raises(ValueError, match="at least one row"):
        m.extend(np.zeros((0, 3)))
    with pytest.raises(ValueError, match="resident=True"):
        m.extend(X, head=_Pair(5, 4))
    with pytest.raises(ValueError, match="head_rows without head"):
        m.extend(X, resident=True, head_rows=[0, 1])
    with pytest.raises(ValueError, match="K = 3"):
        m.extend(X, resident=True, head=_Pair(5, 3))
    for rows in ([0, 5], [-1], [2, 100]):
        with pytest.raises(IndexError, match="outside 0..4"):
            m.extend(X, resident=True, head=_Pair(5, 4), head_rows=rows)
    with pytest.raises(ValueError, match="head pair has been freed"):
        m.extend(X, resident=True, head=_Pair(5, 4, handle=None))
    m.free()
    m.free()                                                   # twice is harmless
    for call in (lambda: m.extend(X), lambda: m.extend(X, resident=True), lambda: m.to_host()):
        with pytest.raises(ValueError, match="freed"):
            call()
    with pytest.raises(ValueError):
        api.heat_kernel_spectrum_model(np.zeros((5, 3)), np.zeros((2, 3)), 4, 2, U=np.zeros((3, 3)))      # U has 3 rows, s = 4


# ------------------------------------------------------------------------------------------- the restatement on the CPU
@pytest.mark.parametrize("gl", npm.GLS)
@pytest.mark.parametrize("root", [False, True])
def test_restated_extension_returns_the_fit_rows_of_an_oracle_fit(oracle, gl, root):
    """an oracle-only fit (the Gram route, stage by stage), its column sums and eigenpairs frozen: the restated extension of
    a shuffled subset of the fit rows is the oracle's vectors of those rows bit for bit.  n = 1500 crosses the 1024-row
    chunk of the column sums; the subset's size differs from n, so a sqrt(n_new) would show."""
    n, d, s, r, K = 1500, 3, 60, 4, 12
    X, U0, U = make_case(n, d, s, r, seed=31)
    fit = npm.oracle_fit(X, U, r, K, gl, root)
    rows = np.random.default_rng(5).permutation(n)[:333]
    vec, val = npm.extend(X[rows], U0, r, gl, fit["colsum_gl"], fit["colsum_spectrum"], fit["sizes"], fit["V"], fit["eig"], n, root)
    np.testing.assert_array_equal(vec, fit["vectors"][rows])
    np.testing.assert_array_equal(val, fit["values"])
    assert np.abs(vec).max() > 0.0
    # and the fit is the oracle's own pipeline: its similarity matrix bit for bit, its heat kernel to rounding
    ei, zn = oracle.cross_similarity(X, U, r, gl=gl)
    a, c2 = oracle.scale_A(ei, zn, s)
    np.testing.assert_array_equal(c2, fit["colsum_spectrum"])
    vals_o, vec_o = oracle.spectrum_from_Z(ei, zn, s, K, root=root, method="gram")
    np.testing.assert_array_equal(vals_o, fit["values"])
    np.testing.assert_allclose(vec_o, fit["vectors"], rtol=0, atol=1e-12 * np.abs(vec_o).max())     # (u / sqrt(n)) * sqrt(n)


def test_restated_scale_is_the_three_passes():
    import np_sparse_stages as nps
    idx, val, sizes = nps.ell_inputs(300, 20, 5, seed=2)
    c1 = nps.colsum(idx, val, 20); c2 = np.linspace(-1.0, 2.0, 20); c2[3] = 0.0
    want = nps.col_scale(idx, nps.row_normalize(nps.col_scale(idx, val, c1, sizes, 0)), c2, None, 1)
    np.testing.assert_array_equal(npm.scale(idx, val, c1, sizes, c2), want)
    np.testing.assert_array_equal(npm.scale(idx, val, None, None, c2), nps.col_scale(idx, nps.row_normalize(val), c2, None, 1))
