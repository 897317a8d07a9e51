"""CPU: the Nystrom-predictor entries (include/flgp_hip.h) are declared, exported and bound, and the refusals
that need no live handle arrive with FLGP_ERR_INVALID and the documented name, *out cleared: a null out, then a null grid.
The next refusal in the order -- the bandwidth index against the grid's l -- reads the grid, so it and everything behind it
(the mirrored entry's refusals, K, the device, the values) are in tests/test_gpu_nystrom_predictor.py on a live grid.
flgp_dev_nystrom_predictor_rows refuses every bad argument before any launch; the entries of the model-backed predictor
still refuse what they refused; the Python class checks its arrays before it touches the library."""
import ctypes
import os
import re

import numpy as np
import pytest

from flgp_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("flgp_predictor_nystrom_regression_create", "flgp_predictor_nystrom_logit_create", "flgp_dev_nystrom_predictor_rows",
         "flgp_dev_nystrom_predictor_workspace")
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
    for method in ("nystrom_regression", "nystrom_logit", "apply", "to_host", "free"):
        assert callable(getattr(api.Predictor, method))


def _regression(grid=None, i=0, out="byref"):
    i0 = np.arange(3, dtype=np.int32); y = np.zeros((3, 1), order="F"); nz = np.full(3, 0.1)
    h = ctypes.c_void_p(1)
    rc = _lib.lib().flgp_predictor_nystrom_regression_create(grid, i, FAKE, 2, i0.ctypes.data, 3, y.ctypes.data, 1, 1.0, nz.ctypes.data,
                                                             1, 1e-3, ctypes.byref(h) if out else None)
    return rc, h.value


def _logit(grid=None, i=0, out="byref"):
    i0 = np.arange(3, dtype=np.int32); y = np.ones((3, 1), order="F"); ts = np.array([1.0])
    h = ctypes.c_void_p(1)
    rc = _lib.lib().flgp_predictor_nystrom_logit_create(grid, i, FAKE, 2, i0.ctypes.data, 3, y.ctypes.data, 1, None, ts.ctypes.data, 1,
                                                        0.0, 1e-3, 1e-5, 10, 0, None, ctypes.byref(h) if out else None)
    return rc, h.value


def test_create_refuses_a_null_out_then_a_null_grid():
    # out comes first: with it null even a non-null grid is not looked at
    assert _regression(grid=FAKE, out=None)[0] == -1 and _message() == "predictor_nystrom_regression: null pointer"
    assert _logit(grid=FAKE, out=None)[0] == -1 and _message() == "predictor_nystrom_logit: null pointer"
    # the grid comes before the bandwidth index and the mirrored entry's checks: i = -1 and a pair that is no pair
    for i in (0, -1):
        rc, h = _regression(i=i)
        assert rc == -1 and _message() == "predictor_nystrom_regression: null grid" and h is None
        rc, h = _logit(i=i)
        assert rc == -1 and _message() == "predictor_nystrom_logit: null grid" and h is None


def _rows(X=FAKE, n=4, ldx=4, d=3, Ut=FAKE, uu=FAKE, U=FAKE, ldu=5, s=5, inv_c=0.5, w=FAKE, P=FAKE, ldp=8, groups=2, K=3, q=1,
          cg=FAKE, mean=FAKE, ldm=4, var=FAKE, ldv=4, work=FAKE, work_bytes=1 << 30):
    return _lib.lib().flgp_dev_nystrom_predictor_rows(None, X, n, ldx, d, Ut, uu, U, ldu, s, inv_c, w, P, ldp, groups, K, q, cg, mean,
                                                      ldm, var, ldv, work, work_bytes)


ROWS_REFUSALS = [
    (dict(X=None), "null pointer"), (dict(Ut=None), "null pointer"), (dict(uu=None), "null pointer"), (dict(U=None), "null pointer"),
    (dict(w=None), "null pointer"), (dict(P=None), "null pointer"), (dict(work=None), "null pointer"),
    (dict(mean=None, var=None), "null pointer (no output is wanted)"), (dict(cg=None), "null pointer (the variance needs cg)"),
    (dict(d=0), "kernels are built for 1 <= d <="), (dict(d=1 << 20), "kernels are built for 1 <= d <="),
    (dict(n=0), "bad shape"), (dict(s=0), "bad shape"), (dict(groups=0), "bad shape"), (dict(K=0), "bad shape"), (dict(q=-1), "bad shape"),
    (dict(q=0), "a mean needs q >= 1"),
    (dict(inv_c=0.0), "inv_c=0 must be positive and finite"), (dict(inv_c=float("nan")), "must be positive and finite"),
    (dict(inv_c=float("inf")), "must be positive and finite"),
    (dict(ldp=7), "ldp=7 is below groups (K + q) = 8"),
    (dict(ldx=3), "leading dimension"), (dict(ldu=4), "leading dimension"), (dict(ldm=3), "leading dimension"),
    (dict(ldv=3), "leading dimension"),
    (dict(work_bytes=64), "the workspace holds 64 bytes"),
]


@pytest.mark.parametrize("kw,text", ROWS_REFUSALS)
def test_row_entry_refuses_before_any_launch(kw, text):
    assert _rows(**kw) == -1
    assert _message().startswith("nystrom_predictor_rows: ") and text in _message(), _message()


def test_workspace_sizes():
    ws = _lib.lib().flgp_dev_nystrom_predictor_workspace
    for bad in ((0, 5, 1, 3, 1, 1), (4, 0, 1, 3, 1, 1), (4, 5, 0, 3, 1, 1), (4, 5, 1, 0, 1, 1), (4, 5, 1, 3, -1, 1)):
        assert ws(*bad) == 0
    mean_only, both = ws(300, 130, 3, 65, 1, 0), ws(300, 130, 3, 65, 1, 1)
    assert mean_only >= 8 * 300 * 130 and both >= mean_only + 8 * 300 * 3 * 66          # Z, and T of all three groups
    assert mean_only % 256 == 0 and both % 256 == 0
    assert _rows(mean=None, work_bytes=ws(4, 5, 2, 3, 1, 0)) == -1 and "are needed" in _message()      # a variance needs T as well


def test_the_model_backed_entries_still_refuse_what_they_refused():
    L = _lib.lib()
    i0 = np.arange(3, dtype=np.int32); y = np.zeros((3, 1), order="F"); nz = np.full(3, 0.1); h = ctypes.c_void_p(1)
    assert L.flgp_predictor_regression_create(None, FAKE, 2, i0.ctypes.data, 3, y.ctypes.data, 1, 1.0, nz.ctypes.data, 1, 1e-3,
                                              ctypes.byref(h)) == -1
    assert _message() == "predictor_regression: null model" and h.value is None
    X = np.zeros((5, 3), order="F"); v = np.zeros(5)
    assert L.flgp_predictor_apply(None, X.ctypes.data, 5, v.ctypes.data, v.ctypes.data) == -1 and _message() == "predictor_apply: null handle"
    assert L.flgp_dev_predictor_apply(None, None, X.ctypes.data, 5, 4, v.ctypes.data, 5, None, 5) == -1 and "leading dimension" in _message()
    assert L.flgp_predictor_dims(None, *[None] * 8) == -1 and _message() == "predictor_dims: null handle"
    assert L.flgp_predictor_to_host(None, None, None) == -1 and _message() == "predictor_to_host: null handle"
    L.flgp_predictor_free(None)


class _Pair:
    def __init__(self, handle=ctypes.c_void_p(0)):
        self._h = handle


def test_python_class_checks_before_the_library():
    grid = api.NystromGrid(ctypes.c_void_p(0), (0.7, 1.0), 10, 3, 4)
    idx0, Y = np.arange(6), np.zeros((6, 2))
    with pytest.raises(TypeError, match="NystromGrid"):
        api.Predictor.nystrom_regression(object(), 0, _Pair(), Y, idx0, 4, (1.0, 0.1), 1e-3)
    for i in (-1, 2):
        with pytest.raises(IndexError, match="outside 0..1"):
            api.Predictor.nystrom_regression(grid, i, _Pair(), Y, idx0, 4, (1.0, 0.1), 1e-3)
    with pytest.raises(ValueError, match="pair has been freed"):
        api.Predictor.nystrom_regression(grid, 0, _Pair(None), Y, idx0, 4, (1.0, 0.1), 1e-3)
    with pytest.raises(ValueError, match="one row per entry of idx0"):
        api.Predictor.nystrom_regression(grid, 0, _Pair(), Y[:5], idx0, 4, (1.0, 0.1), 1e-3)
    with pytest.raises(ValueError, match="one noise variance per training row"):
        api.Predictor.nystrom_regression(grid, 0, _Pair(), Y, idx0, 4, (1.0, 0.1, 0.2), 1e-3, noisepar="different")
    with pytest.raises(api.FlgpError, match="noisepar"):
        api.Predictor.nystrom_regression(grid, 0, _Pair(), Y, idx0, 4, (1.0, 0.1), 1e-3, noisepar="other")
    with pytest.raises(ValueError, match="one entry per value of t"):
        api.Predictor.nystrom_logit(grid, 0, _Pair(), idx0, 4, [1.0, 2.0], Y, col=[0])
    with pytest.raises(ValueError, match="one row per entry of idx0"):
        api.Predictor.nystrom_logit(grid, 0, _Pair(), idx0, 4, [1.0, 2.0], Y[:4])
    grid._h = None                                 # (nothing to free: the handle was never the library's)
    with pytest.raises(ValueError, match="freed"):
        api.Predictor.nystrom_regression(grid, 0, _Pair(), Y, idx0, 4, (1.0, 0.1), 1e-3)
