"""CPU: the regression posterior's entry (flgp_eigenpair_regression_posterior, include/flgp_hip.h) is declared and bound,
and refuses shapes below 1, an n_noise that is neither 1 nor m, a target without nll (and the reverse), a target with
q != 1, a t or sigma that is not finite, null pointers and a call without an output before any device work, so these run
without a GPU; the Python method checks its array lengths before it touches the library."""
import ctypes
import os
import re

import numpy as np
import pytest

from flgp_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "flgp_eigenpair_regression_posterior"
FAKE_PAIR = 8          # a non-null handle: every refusal here comes before the pair is looked at


def _call(ep=FAKE_PAIR, K=2, m=3, mnew=2, q=1, n_noise=1, t=1.0, sigma=1e-3, idx0=True, idx1=True, Y=True, noise=True,
          train=True, test=True, cov=True, target=False, nll=False):
    i0 = np.arange(max(m, 1), dtype=np.int32); i1 = np.arange(max(mnew, 1), dtype=np.int32)
    y = np.zeros((max(m, 1), max(q, 1)), order="F"); nz = np.full(max(m, 1), 0.1)
    tr = np.zeros_like(y); te = np.zeros((max(mnew, 1), max(q, 1)), order="F"); cv = np.zeros(max(mnew, 1))
    tg = np.zeros(max(mnew, 1)); val = ctypes.c_double()
    return _lib.lib().flgp_eigenpair_regression_posterior(
        ep, K, i0.ctypes.data if idx0 else None, m, i1.ctypes.data if idx1 else None, mnew, y.ctypes.data if Y else None, q, t,
        nz.ctypes.data if noise else None, n_noise, sigma, tr.ctypes.data if train else None, te.ctypes.data if test else None,
        cv.ctypes.data if cov else None, tg.ctypes.data if target else None, ctypes.addressof(val) if nll else None)


def _message():
    return _lib.lib().flgp_last_error().decode()


def test_symbol_is_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "flgp_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint %s\s*\(" % NAME, text)
    assert NAME in _lib.declared_symbols() and hasattr(_lib.lib(), NAME)


@pytest.mark.parametrize("kw", [dict(K=0), dict(K=-1), dict(m=0), dict(mnew=0), dict(q=0), dict(m=-3)])
def test_shapes_below_one_are_invalid(kw):
    assert _call(**kw) == -1
    assert _message().startswith("regression_posterior: bad shape")


@pytest.mark.parametrize("n_noise", [0, 2, 4, -1])
def test_n_noise_is_one_or_m(n_noise):
    assert _call(m=3, n_noise=n_noise) == -1
    assert _message() == f"regression_posterior: n_noise={n_noise} must be 1 (\"same\") or m=3 (\"different\")"


def test_target_and_nll_come_together():
    for kw in (dict(target=True), dict(nll=True)):
        assert _call(**kw) == -1
        assert _message() == "regression_posterior: target and nll must be given together"


def test_a_target_needs_one_column():
    assert _call(q=2, target=True, nll=True) == -1
    assert _message() == "regression_posterior: the score takes one column (q=2)"


@pytest.mark.parametrize("kw", [dict(t=float("nan")), dict(t=float("inf")), dict(sigma=float("nan")), dict(sigma=-float("inf"))])
def test_t_and_sigma_are_finite(kw):
    assert _call(**kw) == -1
    assert _message().startswith("regression_posterior: t=") and "must be finite" in _message()


@pytest.mark.parametrize("missing", ["ep", "idx0", "idx1", "Y", "noise"])
def test_null_pointers_are_invalid(missing):
    assert _call(**{missing: None if missing == "ep" else False}) == -1
    assert _message() == "regression_posterior: null pointer"


def test_some_output_is_wanted():
    assert _call(train=False, test=False, cov=False) == -1
    assert _message() == "regression_posterior: null pointer (no output is wanted)"


def test_python_method_checks_lengths_before_the_library():
    rp = object.__new__(api.ResidentEigenPair)                # no handle: reaching the library would fail on it
    idx0, idx1, Y = np.arange(6), np.arange(10, 14), np.zeros((6, 2))
    with pytest.raises(ValueError, match="one row per entry of idx0"):
        rp.regression_posterior(Y[:5], idx0, idx1, 2, (1.0, 0.1), 1e-3)
    with pytest.raises(ValueError, match="one noise variance per training row"):
        rp.regression_posterior(Y, idx0, idx1, 2, (1.0, 0.1, 0.2), 1e-3, noisepar="different")
    with pytest.raises(api.FlgpError, match="noisepar"):
        rp.regression_posterior(Y, idx0, idx1, 2, (1.0, 0.1), 1e-3, noisepar="other")
    with pytest.raises(ValueError, match="one entry per row of idx1"):
        rp.regression_posterior(Y[:, :1], idx0, idx1, 2, (1.0, 0.1), 1e-3, target=np.zeros(3))
    with pytest.raises(ValueError, match="needs a target"):
        rp.regression_posterior(Y, idx0, idx1, 2, (1.0, 0.1), 1e-3, return_posterior=False)
