"""CPU: the Polya-Gamma predictor's entries (include/flgp_hip.h) are declared, exported and bound, and every
refusal made before a handle is read arrives with FLGP_ERR_INVALID, the documented name and in the documented order, *out
cleared; so these run without a GPU.  The order is shown by breaking two things at once: the earlier refusal must win.  What
reads a live handle -- K against the pair's, a pair of another fit, the bandwidth index against the grid's l, `var` on a PG
handle, the C entries on a handle of another kind -- is in tests/test_gpu_predictor_pg.py and
tests/test_gpu_nystrom_predictor_pg.py.  The Python class checks its arrays, and the kind of its handle, before it touches
the library."""
import ctypes
import os
import re

import numpy as np
import pytest

from flgp_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("flgp_predictor_pg_create", "flgp_predictor_nystrom_pg_create", "flgp_predictor_pg_apply", "flgp_dev_predictor_pg_apply",
         "flgp_dev_predictor_pg_rows", "flgp_dev_pg_link")
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
    assert re.search(r"#define\s+FLGP_PREDICTOR_PG\s+2\b", text)
    for method in ("pg", "pg_for_classes", "nystrom_pg", "nystrom_pg_for_classes", "predict"):
        assert callable(getattr(api.Predictor, method))
    assert api.Predictor._KIND[2] == "pg"


def _create(nystrom=False, head=FAKE, i=0, ep=FAKE, K=2, m=3, ncol=2, col=(0, 1), ts=(1.0, 2.0), seeds=(5, 6), B=None, sigma=1e-2,
            n_sample=4, idx0=True, Y=True, y_value=1.0, out="byref"):
    i0 = np.arange(max(m, 1), dtype=np.int32); y = np.full((max(m, 1), max(ncol, 1)), y_value, order="F")
    tsa = np.array(ts, dtype=np.float64) if ts is not None else None
    sd = np.array(seeds, dtype=np.uint64) if seeds is not None else None
    cols = np.array(col, dtype=np.int32) if col is not None else None
    B = (len(ts) if ts is not None else 1) if B is None else B
    h = ctypes.c_void_p(1)
    tail = (ep, K, i0.ctypes.data if idx0 else None, m, y.ctypes.data if Y else None, ncol, cols.ctypes.data if cols is not None else None,
            tsa.ctypes.data if tsa is not None else None, sd.ctypes.data if sd is not None else None, B, sigma, n_sample, 0, None, None,
            ctypes.byref(h) if out else None)
    L = _lib.lib()
    rc = L.flgp_predictor_nystrom_pg_create(head, i, *tail) if nystrom else L.flgp_predictor_pg_create(head, *tail)
    return rc, h.value


# (what is broken, the text)
REFUSALS = [
    (dict(head=None), "{who}: null {what}"),
    (dict(idx0=False), "{who}: null pointer"), (dict(Y=False), "{who}: null pointer"), (dict(ts=None), "{who}: null pointer"),
    (dict(seeds=None), "{who}: null pointer"),
    (dict(B=0), "{who}: bad shape (B=0, m=3, ncol=2)"), (dict(m=0), "{who}: bad shape (B=2, m=0, ncol=2)"),
    (dict(ncol=0), "{who}: bad shape (B=2, m=3, ncol=0)"),
    (dict(n_sample=0), "{who}: N_sample=0 must be at least 1"),
    (dict(col=None, ncol=3), "{who}: col may be NULL only if ncol == B (ncol=3, B=2)"),
    (dict(col=(0, 2)), "chain 1 (t=2, seed=6): {who}: col=2 is outside [0, ncol=2)"),
    (dict(ts=(1.0, float("inf"))), "chain 1 (t=inf, seed=6): {who}: t must be finite"),
    (dict(y_value=1.5), "{who}: Y[0, 0]=1.5 is outside [0, 1]"),
    (dict(sigma=-1.0), "{who}: sigma must be finite and >= 0"), (dict(sigma=float("nan")), "{who}: sigma must be finite and >= 0"),
    (dict(ep=None), "{who}: null eigenpair"),
]


@pytest.mark.parametrize("kw,text", REFUSALS)
def test_create_refuses_before_any_device_work(kw, text):
    rc, h = _create(**kw)
    assert rc == -1 and _message() == text.format(who="predictor_pg", what="model"), _message()
    assert h is None                                           # *out is cleared on every refusal


# the documented order: stage k broken together with every later stage gives stage k's refusal
STAGES = [
    (dict(head=None), "predictor_pg: null model"),
    (dict(idx0=False), "predictor_pg: null pointer"),
    (dict(B=0), "predictor_pg: bad shape (B=0, m=3, ncol=3)"),
    (dict(n_sample=0), "predictor_pg: N_sample=0 must be at least 1"),
    (dict(col=None, ncol=3), "predictor_pg: col may be NULL only if ncol == B (ncol=3, B=2)"),
    (dict(ts=(1.0, float("inf"))), "chain 1 (t=inf, seed=6): predictor_pg: t must be finite"),
    (dict(y_value=1.5), "predictor_pg: Y[0, 0]=1.5 is outside [0, 1]"),
    (dict(sigma=-1.0), "predictor_pg: sigma must be finite and >= 0"),
    (dict(ep=None), "predictor_pg: null eigenpair"),
]


@pytest.mark.parametrize("at", range(len(STAGES)))
def test_create_refuses_in_the_documented_order(at):
    kw = {}
    for later, _ in reversed(STAGES[at:]):
        kw.update(later)
    rc, h = _create(**kw)
    assert rc == -1 and _message() == STAGES[at][1] and h is None, _message()


def test_create_without_out_is_a_null_pointer_before_everything():
    assert _create(out=None, head=None)[0] == -1 and _message() == "predictor_pg: null pointer"
    assert _create(nystrom=True, out=None, head=None)[0] == -1 and _message() == "predictor_nystrom_pg: null pointer"
    rc, h = _create(nystrom=True, head=None, i=-1, ep=None)
    assert rc == -1 and _message() == "predictor_nystrom_pg: null grid" and h is None


def test_apply_refusals():
    L = _lib.lib()
    X = np.zeros((5, 3), order="F"); v = np.zeros(5)
    p = v.ctypes.data
    for args, text in (((None, None, 5, p, p, p, p), "predictor_pg_apply: null pointer"),
                       ((None, X.ctypes.data, 5, None, None, None, None), "predictor_pg_apply: null pointer"),
                       ((None, X.ctypes.data, 0, p, None, None, None), "predictor_pg_apply: need n_new >= 1 (n_new=0)"),
                       ((None, X.ctypes.data, 5, None, None, None, p), "predictor_pg_apply: null handle")):
        assert L.flgp_predictor_pg_apply(*args) == -1 and _message() == text, _message()
    x = X.ctypes.data
    for args, text in (((None, None, None, 5, 5, p, 5, p, 5, p, 5, p), "null pointer"),
                       ((None, None, x, 5, 5, None, 5, None, 5, None, 5, None), "null pointer"),
                       ((None, None, x, 0, 5, p, 5, None, 5, None, 5, None), "need n_new >= 1 (n_new=0)"),
                       ((None, None, x, 5, 4, p, 5, None, 5, None, 5, None), "a leading dimension is below n_new = 5"),
                       ((None, None, x, 5, 5, p, 4, None, 5, None, 5, None), "a leading dimension is below n_new = 5"),
                       ((None, None, x, 5, 5, None, 5, p, 4, None, 5, None), "a leading dimension is below n_new = 5"),
                       ((None, None, x, 5, 5, None, 5, None, 5, p, 4, None), "a leading dimension is below n_new = 5"),
                       ((None, None, x, 5, 5, None, 4, None, 4, None, 4, p), "null handle")):       # an unused ld is not looked at
        assert L.flgp_dev_predictor_pg_apply(*args) == -1 and _message() == "predictor_pg_apply: " + text, _message()


def _rows(idx=FAKE, val=FAKE, n=4, r=2, P=FAKE, ldp=16, s=5, B=3, f=FAKE, ldf=4, pi=FAKE, ldpi=4, y=FAKE, ldy=4, label=FAKE):
    return _lib.lib().flgp_dev_predictor_pg_rows(None, idx, val, n, r, P, ldp, s, B, f, ldf, pi, ldpi, y, ldy, label)


ROWS_REFUSALS = [
    (dict(idx=None), "null pointer"), (dict(val=None), "null pointer"), (dict(P=None), "null pointer"),
    (dict(f=None, pi=None, y=None, label=None), "null pointer (no output is wanted)"),
    (dict(n=0), "bad shape (n=0, r=2, s=5, B=3)"), (dict(r=0), "bad shape"), (dict(r=33), "bad shape"), (dict(s=0), "bad shape"),
    (dict(B=0), "bad shape"),
    (dict(ldp=2), "ldp=2 is below B = 3"),
    (dict(ldf=3), "a leading dimension is below n = 4"), (dict(ldpi=3), "a leading dimension is below n = 4"),
    (dict(ldy=3), "a leading dimension is below n = 4"),
]


@pytest.mark.parametrize("kw,text", ROWS_REFUSALS)
def test_row_kernel_refuses_before_any_launch(kw, text):
    assert _rows(**kw) == -1
    assert _message().startswith("predictor_pg_rows: ") and text in _message(), _message()


def test_row_kernel_refuses_in_the_pattern_of_predictor_rows():
    """null inputs, no output, the shape, ldp, the leading dimensions: each with everything behind it broken as well"""
    chain = [dict(idx=None), dict(f=None, pi=None, y=None, label=None), dict(n=0), dict(ldp=2), dict(ldf=-1, ldpi=-1, ldy=-1)]
    texts = ["null pointer", "null pointer (no output is wanted)", "bad shape (n=0, r=2, s=5, B=3)", "ldp=2 is below B = 3",
             "a leading dimension is below n = 4"]
    for at in range(len(chain)):
        kw = {}
        for later in reversed(chain[at:]):
            kw.update(later)
        if at == len(chain) - 1:
            kw.update(f=FAKE)
        elif at > 1:
            kw.update(f=FAKE, pi=FAKE, y=FAKE, label=FAKE)
        assert _rows(**kw) == -1 and _message() == "predictor_pg_rows: " + texts[at], (at, _message())
    # an output that is not asked for does not need a leading dimension
    assert _rows(f=None, ldf=0, pi=None, ldpi=0, n=0) == -1 and "bad shape" in _message()


def _link(f=FAKE, ldf=4, n=4, B=3, pi=FAKE, ldpi=4, y=FAKE, ldy=4, label=FAKE):
    return _lib.lib().flgp_dev_pg_link(None, f, ldf, n, B, pi, ldpi, y, ldy, label)


LINK_REFUSALS = [
    (dict(f=None), "pg_link: null pointer"),
    (dict(pi=None, y=None, label=None), "pg_link: null pointer (no output is wanted)"),
    (dict(n=0), "pg_link: bad shape (n=0, B=3)"), (dict(B=0), "pg_link: bad shape (n=4, B=0)"),
    (dict(ldf=3), "pg_link: a leading dimension is below n = 4"), (dict(ldpi=3), "pg_link: a leading dimension is below n = 4"),
    (dict(ldy=3), "pg_link: a leading dimension is below n = 4"),
]


@pytest.mark.parametrize("kw,text", LINK_REFUSALS)
def test_link_refuses_before_any_launch(kw, text):
    assert _link(**kw) == -1 and _message() == text, _message()


def test_link_refuses_in_order():
    assert _link(f=None, pi=None, y=None, label=None, n=0, ldf=0) == -1 and _message() == "pg_link: null pointer"
    assert _link(pi=None, y=None, label=None, n=0, ldf=0) == -1 and _message() == "pg_link: null pointer (no output is wanted)"
    assert _link(n=0, ldf=-1) == -1 and _message() == "pg_link: bad shape (n=0, B=3)"
    # an output that is not asked for does not need a leading dimension
    assert _link(pi=None, ldpi=0, y=None, ldy=0, n=0) == -1 and _message() == "pg_link: bad shape (n=0, B=3)"


class _Pair:
    def __init__(self, handle=ctypes.c_void_p(0)):
        self._h = handle


def _handle_of_kind(kind, q=1):
    """a Predictor that never was the library's: what predict checks before it calls it"""
    p = api.Predictor.__new__(api.Predictor)
    p._h = None
    p._model = api.SpectrumModel(ctypes.c_void_p(0), dims=(100, 3, 10, 3, 4, 0, 2, 1))
    p.d, p.s, p.r, p.K, p.groups, p.q, p.kind, p.ldp, p.iters = 3, 10, 3, 4, 1, q, kind, 16, None
    return p


def test_python_class_checks_before_the_library():
    model = api.SpectrumModel(ctypes.c_void_p(0), dims=(100, 3, 10, 3, 4, 0, 2, 1))
    idx0, Y = np.arange(6), np.zeros((6, 2))
    with pytest.raises(TypeError, match="SpectrumModel"):
        api.Predictor.pg(object(), _Pair(), idx0, 2, [1.0, 2.0], Y, 1e-2)
    with pytest.raises(TypeError, match="NystromGrid"):
        api.Predictor.nystrom_pg(object(), 0, _Pair(), idx0, 2, [1.0, 2.0], Y, 1e-2)
    with pytest.raises(ValueError, match="pair has been freed"):
        api.Predictor.pg(model, _Pair(None), idx0, 2, [1.0, 2.0], Y, 1e-2)
    with pytest.raises(ValueError, match="one row per entry of idx0"):
        api.Predictor.pg(model, _Pair(), idx0, 2, [1.0, 2.0], Y[:5], 1e-2)
    with pytest.raises(api.FlgpError, match=r"predictor_pg: col may be NULL only if ncol == B \(ncol=2, B=3\)"):
        api.Predictor.pg(model, _Pair(), idx0, 2, [1.0, 2.0, 3.0], Y, 1e-2)
    with pytest.raises(ValueError, match="col must have one entry per value of t"):
        api.Predictor.pg(model, _Pair(), idx0, 2, [1.0, 2.0], Y, 1e-2, col=[0])
    with pytest.raises(ValueError, match="seeds must have one entry per value of t"):
        api.Predictor.pg(model, _Pair(), idx0, 2, [1.0, 2.0], Y, 1e-2, seeds=[1])
    with pytest.raises(api.FlgpError, match=r"predictor_pg: Y\[2\]=3 is not a class label in 0 .. 2"):
        api.Predictor.pg_for_classes(model, _Pair(), idx0, 2, [1.0, 2.0, 3.0], [0, 1, 3, 0, 1, 2], 1e-2)
    with pytest.raises(ValueError, match="labels must have one entry per row of idx0"):
        api.Predictor.pg_for_classes(model, _Pair(), idx0, 2, [1.0, 2.0], [0, 1, 0], 1e-2)
    grid = api.NystromGrid(ctypes.c_void_p(0), (0.7, 1.0), 10, 3, 4)
    with pytest.raises(IndexError, match="bandwidth index 2 outside 0..1"):
        api.Predictor.nystrom_pg(grid, 2, _Pair(), idx0, 4, [1.0, 2.0], Y, 1e-2)
    with pytest.raises(api.FlgpError, match="predictor_nystrom_pg: Y"):
        api.Predictor.nystrom_pg_for_classes(grid, 0, _Pair(), idx0, 4, [1.0, 2.0], [0, 1, 2, 0, 1, 0], 1e-2)
    grid._h = None


@pytest.mark.parametrize("kind", ["regression", "logit"])
def test_predict_on_a_handle_of_another_kind_is_refused(kind):
    p = _handle_of_kind(kind)
    p._h = ctypes.c_void_p(FAKE)                               # never dereferenced: the kind is looked at first
    with pytest.raises(api.FlgpError, match="predictor_pg_apply: the handle is not a Polya-Gamma one"):
        p.predict(np.zeros((4, 3)))
    p._h = None                                                # (nothing to free)
    with pytest.raises(ValueError, match="freed"):
        p.predict(np.zeros((4, 3)))


def test_predict_checks_its_rows():
    p = _handle_of_kind("pg", q=3)
    p._h = ctypes.c_void_p(FAKE)
    with pytest.raises(ValueError, match="columns"):
        p.predict(np.zeros((4, 4)))
    with pytest.raises(ValueError, match="at least one row"):
        p.predict(np.zeros((0, 3)))
    p._h = None
