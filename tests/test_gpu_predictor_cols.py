"""GPU (-m gpu): flgp_dev_predictor_cols (csrc/predictor_cols.hip) alone, on random ELL rows and a random P in
padded, canaried buffers: ldo > n, a spare output column, and NaN in every column of P outside [c0, c0 + nc).  Shapes:
tests/predictor_draws_cases.py (what they reach: tests/test_predictor_draws_case_table.py).  Per (r, s, nc, c0) the
restatement is computed once, on the 257 rows; a call on n rows must give its first n.

* out is bit for bit the restatement's (tests/np_predictor_draws.py: one chain over a ascending, multiply then add);
* out is bit for bit flgp_dev_predictor_pg_rows's f on the same P (that kernel has no c0: it is handed P + c0);
* rows give the same bits as one call, in two halves and one at a time;
* the inputs and the canaries are untouched.
The knob predictor_cols_tile_min is 1 for this file, so that every width reaches predictor_cols_kernel; the last test serves
widths on both sides of the default (512) at the default and at 1 and asks for the same bits."""
import functools

import numpy as np
import pytest
import torch

import np_predictor_draws as npd
import predictor_draws_cases as pc
from flgp_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NMAX = max(pc.NS)


@pytest.fixture(scope="module", autouse=True)
def tile_kernel_at_every_width():
    """at the default knob these widths go to predictor_pg_rows_kernel: the tile kernel is what this file is about"""
    L = _lib.lib()
    L.flgp_set_tuning(b"predictor_cols_tile_min", 1)
    yield
    L.flgp_set_tuning(b"predictor_cols_tile_min", pc.TILE_MIN)


@functools.lru_cache(maxsize=None)
def _inputs(r, s, nc, c0):
    rng = np.random.default_rng([r, s, nc, c0])
    if r <= s:
        idx = np.sort(np.stack([rng.permutation(s)[:r] for _ in range(NMAX)]), axis=1).astype(np.int32)
    else:
        idx = np.sort(rng.integers(0, s, size=(NMAX, r)), axis=1).astype(np.int32)                # indices repeat
    val = rng.normal(size=(NMAX, r)) * 10.0 ** rng.uniform(-1.0, 1.0, size=(NMAX, r)) / r        # mixed signs and magnitudes
    ldp = c0 + nc + 5
    P = np.full((s, ldp), np.nan)
    P[:, c0:c0 + nc] = rng.normal(size=(s, nc))
    ref = npd.cols(idx, val, P, c0, nc)
    assert not np.isnan(ref).any()
    for a in (idx, val, P, ref):
        a.setflags(write=False)
    return idx, val, P, ldp, ref


class _Dev:
    """the inputs of one (r, s, nc, c0) on the device, uploaded once"""

    def __init__(self, idx, val, P):
        self.idx = torch.from_numpy(np.array(idx)).to(DEV); self.val = torch.from_numpy(np.array(val)).to(DEV)
        self.P = torch.from_numpy(np.array(P)).to(DEV)


def _run(D, i0, n, r, s, ldp, c0, nc):
    """one call on rows [i0, i0 + n); the output sits in NaN with ldo = n + 3 and a spare column"""
    L = _lib.lib()
    ldo = n + 3
    out = torch.full((nc + 1, ldo), float("nan"), dtype=torch.float64, device=DEV)
    rc = L.flgp_dev_predictor_cols(None, D.idx[i0:].data_ptr(), D.val[i0:].data_ptr(), n, r, D.P.data_ptr(), ldp, s, c0, nc,
                                   out.data_ptr(), ldo)
    assert rc == 0, L.flgp_last_error().decode()
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    assert np.isnan(a[:, n:]).all() and np.isnan(a[nc:]).all()                                    # canaries
    return a[:nc, :n].T


def _pg_rows(D, n, r, s, ldp, c0, nc):
    """flgp_dev_predictor_pg_rows asked for f alone on the same P"""
    L = _lib.lib()
    ldf = n + 1
    f = torch.full((nc, ldf), float("nan"), dtype=torch.float64, device=DEV)
    rc = L.flgp_dev_predictor_pg_rows(None, D.idx.data_ptr(), D.val.data_ptr(), n, r, D.P.data_ptr() + 8 * c0, ldp, s, nc, f.data_ptr(),
                                      ldf, None, 0, None, 0, None)
    assert rc == 0, L.flgp_last_error().decode()
    torch.cuda.synchronize()
    return f.cpu().numpy()[:, :n].T


@pytest.mark.parametrize("nc", pc.NCS)
def test_cols_match_the_restatement_and_the_pg_kernel(nc):
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    for r in pc.RS:
        for s in pc.SS:
            for c0 in pc.C0S:
                idx, val, P, ldp, ref = _inputs(r, s, nc, c0)
                D = _Dev(idx, val, P)
                label = f"r={r} s={s} nc={nc} c0={c0}"
                for n in pc.NS:
                    got = _run(D, 0, n, r, s, ldp, c0, nc)
                    np.testing.assert_array_equal(got, ref[:n], err_msg=f"{label} n={n}")
                np.testing.assert_array_equal(_pg_rows(D, NMAX, r, s, ldp, c0, nc), ref, err_msg=f"pg_rows {label}")
                np.testing.assert_array_equal(D.P.cpu().numpy(), P)
                np.testing.assert_array_equal(D.idx.cpu().numpy(), idx); np.testing.assert_array_equal(D.val.cpu().numpy(), val)


@pytest.mark.parametrize("r,s,nc,c0", [(5, 300, 130, 3), (32, 7, 65, 64), (1, 1, 1, 0)])
def test_rows_do_not_depend_on_the_call(r, s, nc, c0):
    idx, val, P, ldp, ref = _inputs(r, s, nc, c0)
    D = _Dev(idx, val, P)
    n = NMAX
    half = 128                                                                                    # two tiles, then two and one row
    two = np.vstack([_run(D, 0, half, r, s, ldp, c0, nc), _run(D, half, n - half, r, s, ldp, c0, nc)])
    np.testing.assert_array_equal(two, ref)
    odd = np.vstack([_run(D, 0, 100, r, s, ldp, c0, nc), _run(D, 100, n - 100, r, s, ldp, c0, nc)])   # halves that split a tile
    np.testing.assert_array_equal(odd, ref)
    for i in (0, 1, 63, 64, 65, 255, 256):
        np.testing.assert_array_equal(_run(D, i, 1, r, s, ldp, c0, nc)[0], ref[i], err_msg=f"row {i} alone")


@pytest.mark.parametrize("nc", pc.ROUTED_NCS)
def test_the_default_routing_gives_the_same_bits(nc):
    r, s, c0, n = 5, 7, 3, 65
    idx, val, P, ldp, ref = _inputs(r, s, nc, c0)
    D = _Dev(idx, val, P)
    L = _lib.lib()
    tile = _run(D, 0, n, r, s, ldp, c0, nc)
    L.flgp_set_tuning(b"predictor_cols_tile_min", pc.TILE_MIN)
    try:
        routed = _run(D, 0, n, r, s, ldp, c0, nc)
    finally:
        L.flgp_set_tuning(b"predictor_cols_tile_min", 1)
    np.testing.assert_array_equal(tile, ref[:n]); np.testing.assert_array_equal(routed, ref[:n])
