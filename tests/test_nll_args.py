"""CPU: the negative-log-likelihood entries (include/flgp_hip.h) are declared, exported and bound, and
refuse bad arguments before any device work, so these run without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from flgp_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("flgp_negative_log_likelihood", "flgp_dev_nll_workspace", "flgp_dev_nll_classification", "flgp_dev_nll_regression")


def _p(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data


def test_nll_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flgp_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(L, name), name
        assert name in _lib.declared_symbols(), name
    _lib.lib()
    assert callable(api.negative_log_likelihood) and callable(api.nll_classification)


def test_workspace_size():
    ws = _lib.lib().flgp_dev_nll_workspace
    assert ws(1, 1) == 8 * 3                                  # one term, one slab partial, one class value
    assert ws(4096, 1) == 8 * (4096 + 1 + 1)
    assert ws(4097, 3) == 8 * 3 * (4097 + 2 + 1)
    assert ws(0, 1) == 0 and ws(5, 0) == 0


def _refused(rc, what):
    assert rc == -1, rc
    assert what in _lib.lib().flgp_last_error().decode()


def _call(mean=(0.0, 1.0, 2.0), cov=(1.0, 1.0, 1.0), target=(0.0, 1.0, 1.0), n=3, J=1, type="binary", n_samples=100,
          nll=True, like=False):
    mean = None if mean is None else np.asarray(mean, dtype=np.float64)
    cov = None if cov is None else np.asarray(cov, dtype=np.float64)
    target = None if target is None else np.asarray(target, dtype=np.float64)
    out = ctypes.c_double()
    lk = np.zeros(max(n * J, 1)) if like else None
    return _lib.lib().flgp_negative_log_likelihood(_p(mean), _p(cov), _p(target), n, J, None if type is None else type.encode(),
                                                   n_samples, 1, ctypes.addressof(out) if nll else None, _p(lk))


@pytest.mark.parametrize("type", ["regression", "binary", "multinomial"])
def test_null_pointers_and_shapes(type):
    J, target = (2, (0.0, 1.0, 1.0)) if type == "multinomial" else (1, (0.0, 1.0, 1.0))
    mean = np.zeros(3 * J); cov = np.ones(3 * J)
    _refused(_call(mean=None, cov=cov, target=target, J=J, type=type), "null pointer")
    _refused(_call(mean=mean, cov=None, target=target, J=J, type=type), "null pointer")
    _refused(_call(mean=mean, cov=cov, target=None, J=J, type=type), "null pointer")
    _refused(_call(mean=mean, cov=cov, target=target, J=J, type=type, nll=False), "null pointer")
    _refused(_call(mean=mean, cov=cov, target=target, J=J, type=type, n=0), "bad shape")
    _refused(_call(mean=mean, cov=cov, target=target, J=0, type=type), "bad shape")
    _refused(_call(mean=mean, cov=cov, target=target, J=-1, type=type, n=-3), "bad shape")


def test_unknown_type():
    _refused(_call(type="poisson"), "The type of likelihood is not supported!")
    _refused(_call(type=""), "is not supported!")
    _refused(_call(type="Binary"), "is not supported!")
    _refused(_call(type=None), "null pointer")


@pytest.mark.parametrize("type", ["binary", "multinomial"])
@pytest.mark.parametrize("n_samples", [0, -5])
def test_n_samples(type, n_samples):
    J = 2 if type == "multinomial" else 1
    _refused(_call(mean=np.zeros(3 * J), cov=np.ones(3 * J), J=J, type=type, n_samples=n_samples), "n_samples")


@pytest.mark.parametrize("type", ["regression", "binary"])
def test_one_column_types(type):
    _refused(_call(mean=np.zeros(6), cov=np.ones(6), J=2, type=type), "takes one column")


@pytest.mark.parametrize("target,J,what", [
    ((0.0, 1.5, 1.0), 2, "class label"),
    ((0.0, -1.0, 1.0), 2, "class label"),
    ((0.0, 2.0, 1.0), 2, "class label"),           # J = 2 columns: labels 0 and 1
    ((0.0, np.nan, 1.0), 2, "class label"),
    ((0.0, np.inf, 1.0), 2, "class label"),
    ((0.0, 1.0, 1.0), 3, "name 2 classes"),        # max(label) + 1 != J
    ((0.0, 0.0, 0.0), 2, "name 1 classes"),
])
def test_multinomial_labels(target, J, what):
    _refused(_call(mean=np.zeros(3 * J), cov=np.ones(3 * J), target=target, J=J, type="multinomial", like=True), what)


def test_device_entries_refuse_before_any_launch():
    L = _lib.lib()
    a = np.zeros(8)
    p = _p(a)
    _refused(L.flgp_dev_nll_classification(None, None, p, p, 1, 1, 0, 100, 1, 0, None, p, p), "null pointer")
    _refused(L.flgp_dev_nll_classification(None, p, p, p, 1, 1, 0, 100, 1, 0, None, None, p), "null pointer")
    _refused(L.flgp_dev_nll_classification(None, p, p, p, 1, 1, 0, 100, 1, 0, None, p, None), "null pointer")
    _refused(L.flgp_dev_nll_classification(None, p, p, p, 0, 1, 0, 100, 1, 0, None, p, p), "bad shape")
    _refused(L.flgp_dev_nll_classification(None, p, p, p, 1, 0, 0, 100, 1, 0, None, p, p), "bad shape")
    _refused(L.flgp_dev_nll_classification(None, p, p, p, 1, 1, 0, 0, 1, 0, None, p, p), "n_samples")
    _refused(L.flgp_dev_nll_regression(None, p, None, p, 1, None, p, p), "null pointer")
    _refused(L.flgp_dev_nll_regression(None, p, p, p, 0, None, p, p), "bad shape")


def test_wrapper_shape_errors():
    y = np.array([0.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        api.negative_log_likelihood(np.zeros(2), np.ones(3), y, "binary", seed=1)
    with pytest.raises(ValueError):
        api.negative_log_likelihood(np.zeros(3), np.ones(4), y, "regression")
    with pytest.raises(ValueError):
        api.negative_log_likelihood(np.zeros((3, 2)), np.ones((3, 2)), y, "binary", seed=1)
    with pytest.raises(ValueError):
        api.nll_classification(np.zeros(4), np.ones(4), y, seed=1)
    with pytest.raises(ValueError):
        api.negative_log_likelihood(np.zeros(3), np.ones(3), y, "multinomial", seed=1)          # vectors, not n x J
    with pytest.raises(ValueError):
        api.negative_log_likelihood(np.zeros((2, 2)), np.ones((2, 2)), y, "multinomial", seed=1)
    with pytest.raises(ValueError):
        api.negative_log_likelihood(np.zeros((3, 2)), np.ones((3, 3)), y, "multinomial", seed=1)


def test_wrapper_refusals_reach_the_caller():
    y = np.array([0.0, 1.0, 1.0])
    with pytest.raises(api.FlgpError) as e:
        api.negative_log_likelihood(np.zeros(3), np.ones(3), y, "poisson", seed=1)
    assert e.value.code == -1 and "not supported" in e.value.message
    with pytest.raises(api.FlgpError) as e:
        api.nll_classification(np.zeros(3), np.ones(3), y, n_samples=0, seed=1)
    assert e.value.code == -1
    with pytest.raises(api.FlgpError) as e:
        api.negative_log_likelihood(np.zeros((3, 3)), np.ones((3, 3)), y, "multinomial", seed=1)     # labels name 2 classes
    assert e.value.code == -1 and "classes" in e.value.message
