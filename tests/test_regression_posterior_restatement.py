"""CPU: the weight-space form of the regression posterior (tests/np_regression_posterior.py, what
flgp_eigenpair_regression_posterior computes for m > K) against the oracle's three reference-form functions
on the problems of the GPU test (tests/regression_posterior_cases.py), under the project's tolerances for these quantities
(tests/test_gpu_parity.py: 1e-9 max|ref| for the mean, 1e-9 max|ref| + 2e-15 prior m / (noise + sigma) for the variance);
and var >= noise[0] + sigma exactly."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_regression_posterior as ws  # noqa: E402
import regression_posterior_cases as cases  # noqa: E402


@pytest.mark.parametrize("style", list(cases.STYLES))
@pytest.mark.parametrize("K,m,q", cases.GRID + cases.TILE)
def test_weight_space_form_against_the_reference_form(K, m, q, style):
    values, V = cases.host_pair()
    p = cases.problem(K, m, q, style)
    t, sigma, nz = p["t"], p["sigma"], p["nz"]
    for model, noise in (("same", nz[0]), ("different", nz)):
        for which, idx1 in ((model, p["idx1"]), ("train_" + model, p["idx0"])):
            got = ws.weight_space_mean(values, V, p["Y"], p["idx0"], idx1, K, t, noise, sigma)
            d = np.abs(got - p[which]).max()
            print(f"{which}: |dmean| {d:.3e} (atol {cases.atol_mean(p[which]):.3e})")
            assert d <= cases.atol_mean(p[which]), which
    var = ws.weight_space_variance(values, V, p["idx0"], p["idx1"], K, t, nz[0], sigma)
    d = np.abs(var - p["var"]).max()
    print(f"var: |dvar| {d:.3e} (atol {cases.atol_var(p):.3e})")
    assert d <= cases.atol_var(p)
    assert (var >= p["c"]).all()


def test_different_with_equal_variances_is_same():
    values, V = cases.host_pair()
    p = cases.problem(64, 133, 2, "perm_overlap")
    same = ws.weight_space_mean(values, V, p["Y"], p["idx0"], p["idx1"], 64, p["t"], 0.2, p["sigma"])
    diff = ws.weight_space_mean(values, V, p["Y"], p["idx0"], p["idx1"], 64, p["t"], np.full(133, 0.2), p["sigma"])
    assert np.abs(same - diff).max() <= 1e-9 * np.abs(same).max()
