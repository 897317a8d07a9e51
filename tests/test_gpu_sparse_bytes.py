"""GPU (-m gpu): U-recovery from LDS-resident column slices (route 4 of flgp_dev_u_recover_route, csrc/sparse.hip)
delivers the bits of the gather kernels it stands in for, held to the numpy restatement of tests/np_sparse_stages.py:
at the row count where the entry point starts to take it (found by asking the route query, so that the test follows the
measured crossover), at the s where the slice width changes, K below, at and off a multiple of the width, r from 1 to
FLGP_RMAX, ragged last waves, zero eigenvalues, both `root` settings, with and without the values output."""
import functools
import math

import numpy as np
import pytest
import torch

import np_sparse_stages as nps
from flgp_amd.pipeline import HipStages

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLGP_OK = 0
ROUTE_LDS = 4


@pytest.fixture(scope="module")
def stages():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    return HipStages(DEV)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)            # (a copy: the shared inputs are read-only)


def nan_buffer(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)


# ============================================================================================================ U-recovery
def lds_threshold(stages, r, s, K):
    """the smallest n the entry point serves from LDS slices, by bisection over the route query"""
    route = lambda n: stages.L.flgp_dev_u_recover_route(n, r, s, K, 1)      # noqa: E731
    hi = 1 << 24
    assert route(hi) == ROUTE_LDS and route(1) != ROUTE_LDS
    lo = 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if route(mid) == ROUTE_LDS else (mid, hi)
    return hi


def run_u_recover(stages, idx, val, V, eig, scale, root, want_values=True):
    """flgp_dev_u_recover with the workspace, V held with ldv = s + 3 and the output with ldo = n + 5 and a column too
    many, everything around them NaN.  Returns (vectors buffer (K + 1, ldo), values buffer (K + 1) or None)."""
    n, r = idx.shape
    s, K = V.shape
    ldv, ldo = s + 3, n + 5
    dV = nan_buffer(K, ldv)
    dV[:, :s] = dev(np.asarray(V).T)
    out = nan_buffer(K + 1, ldo)
    values = nan_buffer(K + 1) if want_values else None
    d_idx, d_val, d_eig = dev(idx), dev(val), dev(eig)
    work = stages.empty((stages.L.flgp_dev_u_recover_workspace(s, K) // 8 + 1,))
    rc = stages.L.flgp_dev_u_recover(stages._st(), d_idx.data_ptr(), d_val.data_ptr(), n, r, dV.data_ptr(), ldv, s, d_eig.data_ptr(),
                                     K, float(scale), int(root), out.data_ptr(), ldo, values.data_ptr() if want_values else None,
                                     work.data_ptr())
    stages.sync()
    assert rc == FLGP_OK, stages.L.flgp_last_error()
    return out.cpu().numpy(), (values.cpu().numpy() if want_values else None)


def check_u_recover(stages, idx, val, V, eig, scale, root, want_values=True, lds=True):
    n, r = idx.shape
    s, K = V.shape
    assert (stages.L.flgp_dev_u_recover_route(n, r, s, K, 1) == ROUTE_LDS) == lds
    out, values = run_u_recover(stages, idx, val, V, eig, scale, root, want_values)
    ref, ref_values = nps.u_recover(idx, val, V, eig, scale, root=bool(root))
    assert np.array_equal(out[:K, :n], ref.T)                               # bit for bit
    assert np.isnan(out[:K, n:]).all(), "rows past n were written"
    assert np.isnan(out[K]).all(), "a column past K was written"
    if want_values:
        assert np.array_equal(values[:K], ref_values)
        assert np.isnan(values[K]), "values past K were written"
    return out[:K, :n]


@functools.lru_cache(maxsize=None)
def _inputs(K, n, r, s, seed=0):
    arrays = nps.u_recover_inputs(K, n, r, s, seed)
    for a in arrays:
        a.setflags(write=False)
    assert arrays[0][0, 0] == 0 and arrays[0][n - 1, r - 1] == s - 1          # anchor 0 and anchor s - 1 are there
    return arrays


def test_u_recover_lds_at_the_threshold(stages):
    """the last n of the gather kernels and the first of the LDS kernel on the same rows: the restatement's bits on both
    sides, and the shared rows agree"""
    K, r, s = 5, 3, 97
    T = lds_threshold(stages, r, s, K)
    idx, val, V, eig = _inputs(K, T, r, s)
    above = check_u_recover(stages, idx, val, V, eig, math.sqrt(T), 1)
    below = check_u_recover(stages, idx[:T - 1], val[:T - 1], V, eig, math.sqrt(T), 1, lds=False)
    assert np.array_equal(above[:, :T - 1], below)


@pytest.mark.parametrize("s,lds", [(5120, True), (5121, True), (6826, True), (6827, True), (10240, True), (10241, True),
                                   (20480, True), (20481, False)])
def test_u_recover_lds_slice_width_edges(stages, s, lds):
    """w = min(4, 163840 // (8 s)): the last s of every width (the LDS exactly full at 5120, 10240 and 20480) and the first
    of the next; past 20480 not one column fits and the gather kernels serve the call"""
    K, r = 5, 3
    T = lds_threshold(stages, r, 97, K)
    idx, val, V, eig = _inputs(K, T, r, s)
    check_u_recover(stages, idx, val, V, eig, 1000.0 / 3.0, 0, lds=lds)


@pytest.mark.parametrize("K", [1, 3, 4, 5, 200, 202])
def test_u_recover_lds_slice_counts(stages, K):
    """fewer columns than a slice holds, a ragged last slice, whole slices"""
    r, s = 10, 97
    T = lds_threshold(stages, r, s, K)
    idx, val, V, eig = _inputs(K, T, r, s)
    check_u_recover(stages, idx, val, V, eig, math.sqrt(T), 1)


@pytest.mark.parametrize("r", [1, 10, 32])
@pytest.mark.parametrize("extra", [1, 63])
def test_u_recover_lds_r_and_ragged_rows(stages, r, extra):
    """one entry, a whole chunk of eight and a pair, four whole chunks; a last wave of one row and of 63; with ldo = n + 5
    and ldv = s + 3 as everywhere in this file"""
    K, s = 5, 97
    n = lds_threshold(stages, r, s, K) + extra
    idx, val, V, eig = _inputs(K, n, r, s)
    check_u_recover(stages, idx, val, V, eig, math.sqrt(n), 0, want_values=False)
    check_u_recover(stages, idx, val, V, eig, math.sqrt(n), 1, want_values=True)


def test_u_recover_lds_zero_sigma_columns(stages):
    """eigenvalues 0.0 and -0.0: those columns exactly +0.0, the others the restatement's"""
    K, r, s = 6, 10, 97
    T = lds_threshold(stages, r, s, K)
    idx, val, V, eig = _inputs(K, T, r, s)
    eig = eig.copy()
    eig[[1, 4]] = [0.0, -0.0]
    for root in (0, 1):
        out = check_u_recover(stages, idx, val, V, eig, 1000.0 / 3.0, root)
        assert (out[[1, 4]] == 0.0).all() and not np.signbit(out[[1, 4]]).any()
        assert (np.abs(out[[0, 2, 3, 5]]).max(axis=1) > 0).all()
