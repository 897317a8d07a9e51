"""CPU: the numpy restatement of the GLGP spectrum step (tests/np_glgp.py, reference src/Fit.cpp:383-449) and the
properties the device route leans on: r, the symmetry of W, its spectrum inside (-1, 1), r = n being
"keep everything", and the (tau, jcut) rule reproducing the stable-argsort mask when ties straddle the r-th place."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_glgp as G  # noqa: E402

from flgp_amd import _lib  # noqa: E402


@pytest.mark.parametrize("thr,n", [(0.025, 100), (0.035, 100), (0.004, 100)])     # thr n = 2.5, 3.5, 0.4
def test_neighbours_round_half_up_and_floor_of_three(thr, n):
    want = max(int(np.floor(thr * n + 0.5)), 3)
    assert _lib.lib().flgp_glgp_neighbours(thr, n) == want == G.neighbours(thr, n)


def test_neighbours_values():
    L = _lib.lib()
    assert L.flgp_glgp_neighbours(0.025, 100) == 3       # 2.5 rounds to 3
    assert L.flgp_glgp_neighbours(0.035, 100) == 4       # 3.5 rounds to 4: half away from zero, not to even
    assert L.flgp_glgp_neighbours(0.004, 100) == 3
    assert L.flgp_glgp_neighbours(0.01, 2100) == 21 and L.flgp_glgp_neighbours(0.05, 520) == 26


@pytest.mark.parametrize("sparse", [True, False])
def test_w_is_symmetric_with_spectrum_inside_the_open_interval(sparse):
    X = np.random.default_rng(0).normal(size=(120, 3))
    Dt = G.distances_t(X)
    r = G.neighbours(0.1, 120)
    M = G.kept_mask(Dt, r) if sparse else np.ones_like(Dt, dtype=bool)
    mean = G.kept_sums(Dt, M).sum() / (120 * r) if sparse else Dt.mean()
    for a2 in (0.5, 1.0, 10.0):
        Z = G.similarity(Dt, M, 1.0 / (a2 * mean))
        assert np.array_equal(Z, Z.T)                    # the addition commutes
        W, _ = G.normalise(Z)
        assert np.abs(W - W.T).max() <= 4 * np.finfo(float).eps * np.abs(W).max()
        lam = np.linalg.eigvalsh(0.5 * (W + W.T))
        assert -1.0 < lam[0] and lam[-1] < 1.0
        if sparse:
            assert lam[0] < 0.0                          # indefinite: why the device route shifts
            lam_s = np.linalg.eigvalsh(0.5 * (0.5 * (W + W.T) + np.eye(120)))
            assert 0.0 < lam_s[0] and lam_s[-1] < 1.0
            np.testing.assert_allclose(2.0 * lam_s - 1.0, lam, atol=1e-14)
        else:
            assert lam[0] > -1e-12                       # PSD: not shifted


def test_r_equal_n_keeps_everything():
    X = np.random.default_rng(1).normal(size=(40, 2))
    Dt = G.distances_t(X)
    Dt = 0.5 * (Dt + Dt.T)                               # one orientation, so that the two routes see the same numbers
    assert G.kept_mask(Dt, 40).all()
    (sp,), mean_s, r = G.spectrum(X, 5, (1.0,), sparse=True, threshold=1.0, Dt=Dt)
    (de,), mean_d, _ = G.spectrum(X, 5, (1.0,), sparse=False, Dt=Dt)
    assert r == 40
    np.testing.assert_allclose(mean_s, mean_d, rtol=1e-14)
    np.testing.assert_allclose(sp[0], de[0], rtol=1e-12)


def _tied_matrix():
    rng = np.random.default_rng(5)
    n = 12
    Dt = np.round(rng.uniform(0.0, 4.0, size=(n, n)), 0)       # values 0..4: every list is full of ties
    Dt[:, 3] = 2.0                                            # an all-equal list
    Dt[0, 4] = -0.0; Dt[5, 4] = 0.0; Dt[7, 4] = -1e-17        # signed zeros and a tiny negative
    return Dt


@pytest.mark.parametrize("r", [1, 3, 5, 11, 12])
def test_tau_jcut_rule_reproduces_the_argsort_mask_across_ties(r):
    Dt = _tied_matrix()
    M = G.kept_mask(Dt, r)
    assert (M.sum(axis=0) == r).all()
    tau, jcut = G.tau_jcut(Dt, r)
    assert np.array_equal(G.mask_from_rule(Dt, tau, jcut), M)
    # the ties straddle the r-th place somewhere: the value rule alone keeps too many
    if r in (3, 5):
        assert ((Dt <= tau[None, :]).sum(axis=0) > r).any()
    # ties go to the lower row
    i = 3
    assert np.array_equal(np.flatnonzero(M[:, i]), np.arange(r)) and jcut[i] == r - 1


def test_kept_sums_add_in_ascending_row_order():
    Dt = np.array([[1e16, 0.0, 0.0], [1.0, 0.0, 0.0], [-1e16, 0.0, 0.0]])
    M = np.ones((3, 3), dtype=bool)
    assert G.kept_sums(Dt, M)[0] == (1e16 + 1.0) + -1e16                  # 0.0, not the 1.0 of another order
