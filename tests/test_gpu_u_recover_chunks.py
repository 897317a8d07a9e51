"""GPU (-m gpu): the step shapes of u_recover_lds_kernel (csrc/sparse.hip).  A lane walks its row in steps of NP pairs of
entries, NP cut to the row: the fewest steps of at most six pairs, all of one size (u_lds_pairs) --

    r      1-2  3-4  5-6  7-8  9-10  11-12  13-16  17-20  21-24  25-30  31-32
    steps   1    1    1    1    1      1      2      2      2      3      3
    NP      1    2    3    4    5      6      4      5      6      5      6

so the r below take every NP, whole and ragged last steps, and at odd r the pair of the row's last slot, which reaches into
the next row and is moved back in the last row of all.  V must be the numpy restatement's (tests/np_sparse_stages.py:
a ascending, multiply then add, (acc / sigma) * scale) bit for bit, through flgp_dev_u_recover on the LDS route, with
ldv = s + 3 and ldo = n + 5 and NaN around everything."""
import functools
import math

import numpy as np
import pytest
import torch

import np_sparse_stages as nps
from flgp_amd.pipeline import HipStages

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROUTE_LDS = 4
THREADS = 1024                   # lanes of a workgroup = rows of one step
RS = [1, 2, 4, 6, 7, 8, 9, 10, 11, 15, 16, 17, 24, 25, 31, 32]


def pairs_per_step(r):
    pairs = (r + 1) // 2
    steps = -(-pairs // 6)
    return -(-pairs // steps), steps


def test_the_r_list_takes_every_step_shape():
    shapes = {pairs_per_step(r) for r in RS}
    assert {np_ for np_, _ in shapes} == {1, 2, 3, 4, 5, 6} and {st for _, st in shapes} == {1, 2, 3}
    assert pairs_per_step(10) == (5, 1) and pairs_per_step(16) == (4, 2) and pairs_per_step(32) == (6, 3)
    assert any(r % 2 for r in RS if pairs_per_step(r)[1] == 1) and any(r % 2 for r in RS if pairs_per_step(r)[1] > 1)


@pytest.fixture(scope="module")
def stages():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    return HipStages(DEV)


@functools.lru_cache(maxsize=None)
def case(K, n, r, s):
    """(idx, val, V, eig, reference vectors n x K) -- read-only, shared"""
    idx, val, V, eig = nps.u_recover_inputs(K, n, r, s, 0)
    ref, _ = nps.u_recover(idx, val, V, eig, math.sqrt(n))
    for a in (idx, val, V, eig, ref):
        a.setflags(write=False)
    return idx, val, V, eig, ref


def run(stages, idx, val, V, eig, scale):
    n, r = idx.shape
    s, K = V.shape
    assert stages.L.flgp_dev_u_recover_route(n, r, s, K, 1) == ROUTE_LDS
    ldv, ldo = s + 3, n + 5
    dV = torch.full((K, ldv), float("nan"), dtype=torch.float64, device=DEV)
    dV[:, :s] = torch.from_numpy(np.ascontiguousarray(np.asarray(V).T)).to(DEV)
    out = torch.full((K + 1, ldo), float("nan"), dtype=torch.float64, device=DEV)
    d_idx, d_val, d_eig = (torch.from_numpy(np.array(a, order="C")).to(DEV) for a in (idx, val, eig))
    work = stages.empty((stages.L.flgp_dev_u_recover_workspace(s, K) // 8 + 1,))
    rc = stages.L.flgp_dev_u_recover(stages._st(), d_idx.data_ptr(), d_val.data_ptr(), n, r, dV.data_ptr(), ldv, s, d_eig.data_ptr(),
                                     K, float(scale), 0, out.data_ptr(), ldo, None, work.data_ptr())
    stages.sync()
    assert rc == 0, stages.L.flgp_last_error()
    out = out.cpu().numpy()
    assert np.isnan(out[:K, n:]).all(), "rows past n were written"
    assert np.isnan(out[K]).all(), "a column past K was written"
    return out[:K, :n]


@pytest.mark.parametrize("n", [10000, 10001])
@pytest.mark.parametrize("r", RS)
def test_every_step_shape(stages, r, n):
    """K = 5: a whole slice of four eigen-columns and a ragged one.  256 CUs / 2 slices: ranges of 128 rows, so every range
    ends inside a step of 1024 lanes, and the last one (16 or 17 rows) inside a wave."""
    idx, val, V, eig, ref = case(5, n, r, 64)
    assert np.array_equal(run(stages, idx, val, V, eig, math.sqrt(n)), ref.T)


@pytest.mark.parametrize("s", [64, 5000])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 200])
@pytest.mark.parametrize("r", [10, 11])
def test_slices_and_ranges(stages, r, K, s):
    """one step of five pairs and one of six with a ragged pair (odd r: the moved pair of the last row), fewer columns than a
    slice, ragged and whole slices; at K = 200 the fifty slices leave five ranges of 2048 rows, which a lane walks in two
    steps, the last range (1809 rows) ending inside its second"""
    n = 10001
    idx, val, V, eig, ref = case(K, n, r, s)
    assert np.array_equal(run(stages, idx, val, V, eig, math.sqrt(n)), ref.T)


def test_rows_per_range_of_the_cases_above():
    """the launch rule of u_recover_lds_launch on 256 compute units: what the two docstrings above say about the ranges"""
    def ranges(n, K, cus=256):
        ceil = lambda a, b: -(-a // b)                                                 # noqa: E731
        rows = ceil(ceil(n, max(cus // ceil(K, 4), 1)), 64) * 64
        return rows, n - (ceil(n, rows) - 1) * rows
    assert ranges(10000, 5) == (128, 16) and ranges(10001, 5) == (128, 17)
    rows, last = ranges(10001, 200)
    assert rows == 2 * THREADS and THREADS < last < rows and last % 64


@pytest.mark.parametrize("r", [9, 10, 17])
def test_zero_sigma_column(stages, r):
    n, K = 10001, 6
    idx, val, V, eig, _ = case(K, n, r, 64)
    eig = eig.copy()
    eig[[1, 4]] = [0.0, -0.0]
    ref, _ = nps.u_recover(idx, val, V, eig, 1000.0 / 3.0)
    out = run(stages, idx, val, V, eig, 1000.0 / 3.0)
    assert np.array_equal(out, ref.T)
    assert (out[[1, 4]] == 0.0).all() and not np.signbit(out[[1, 4]]).any()
    assert (np.abs(out[[0, 2, 3, 5]]).max(axis=1) > 0).all()
