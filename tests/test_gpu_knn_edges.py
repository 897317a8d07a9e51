"""GPU: flgp_dev_knn at every cell of its dispatcher and at the tile, workgroup and stride edges of its kernels.

flgp_dev_knn picks one of 63 template instantiations from (d, r, s) and three tuning switches.  knn_cases.route restates that
choice; test_knn_case_table.py (CPU) shows with it that the table reaches every instantiation and every edge, and the id of each
test here names the cell it runs.

Every case goes through ctypes to flgp_dev_anchor_prep and flgp_dev_knn on padded buffers (knn_cases.Placement): X and U with
leading dimensions n + 3 and s + 3, their pad columns NaN; the outputs (r + 1) x (n + 5) in buffers of canaries.  The bar is
the project's for this stage, and there is nothing to choose in it: indices equal the oracle's, distances equal the oracle's
bit for bit (compared as uint64), and every element outside the first r rows x n columns of both outputs still holds its
canary bit pattern.  Each case runs a second time without a distance buffer: same indices, and the distance buffer lying
alongside stays all canary.

Which path a constructed case takes inside a kernel -- a drain on every step, a screen queue exactly full, one entry more and a
rescan by the whole wave -- follows from its construction (knn_cases.approach, copies, origin); only results are observable.
For the same reason two boundaries cannot be pinned from outside: draining a queue one step early (`cnt > QC - A` read as
`>=`) and rescanning a point whose screen queue is exactly full (`c0 > QC` read as `>=`) are both exact, so they return the
same bits; the opposite slips would write or read past the queue in LDS.  (That the constructions take the paths they claim
showed once by hand: with the screen's merge of its two half-queues turned round, copies(256) failed -- its points went through
the exactly full queue -- while copies(264) and copies(768), which rescan, still passed.)

Measured on an MI355X: the whole file (243 tests) 2.6 s, the slowest test 0.17 s (the first one, which loads the library); the
two rows at s = 32768 / 32769 take 0.03 - 0.04 s each.  Every case passed as the kernels stood."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_cases as K  # noqa: E402
from flgp_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLGP_OK, FLGP_ERR_INVALID = 0, -1


@pytest.fixture(scope="module")
def L(oracle):
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


class tuned:
    """the row's tuning switches for the duration of a block; every switch back at its default afterwards"""

    def __init__(self, L, tuning):
        self.L, self.tuning = L, tuning

    def __enter__(self):
        for key, value in self.tuning.items():
            self.L.flgp_set_tuning(key.encode(), value)

    def __exit__(self, *exc):
        for key, value in K.DEFAULTS.items():
            self.L.flgp_set_tuning(key.encode(), value)


def placed(L, X, U, r):
    """the buffers of one problem, the anchor panel prepared from the padded U"""
    n, d = X.shape
    s = U.shape[0]
    pl = K.Placement(X, U, r, L.flgp_dev_anchor_rows(s), L.flgp_dev_anchor_dpad(d), DEV)
    _lib.check(L.flgp_dev_anchor_prep(stream(), pl.U.data_ptr(), s, pl.ldu, d, pl.Ut.data_ptr(), pl.uu.data_ptr()))
    return pl


def knn(L, pl, with_dist=True, **over):
    """one flgp_dev_knn on the placement's buffers; `over` replaces arguments (the refusals)"""
    a = dict(n=pl.n, ldx=pl.ldx, d=pl.d, s=pl.s, r=pl.r, ldo=pl.ldo)
    a.update(over)
    rc = L.flgp_dev_knn(stream(), pl.X.data_ptr(), a["n"], a["ldx"], a["d"], pl.Ut.data_ptr(), pl.uu.data_ptr(), a["s"], a["r"],
                        pl.idx.data_ptr(), pl.dist.data_ptr() if with_dist else None, a["ldo"])
    torch.cuda.synchronize()
    return rc


def run_twice(L, case, X, U):
    """(indices, distance bits) of the call with a distance buffer, after the checks both calls share: the canaries around the
    results, and the same indices from the call without a distance buffer"""
    with tuned(L, case.tuning):
        pl = placed(L, X, U, case.r)
        _lib.check(knn(L, pl))
        idx, bits = pl.read()
        assert pl.idx_untouched(), "a store outside the r x n block of the indices (the extra row, or the pad of ldo)"
        assert pl.dist_untouched(), "a store outside the r x n block of the distances (the extra row, or the pad of ldo)"
        pl.fresh_outputs()
        _lib.check(knn(L, pl, with_dist=False))
        idx2, _ = pl.read()
        assert pl.idx_untouched(), "without a distance buffer: a store outside the r x n block of the indices"
        assert pl.dist_untouched(whole=True), "without a distance buffer: a store into the distance buffer nobody named"
    np.testing.assert_array_equal(idx2, idx, err_msg="the indices differ between the calls with and without distances")
    return idx, bits


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_case(L, case):
    """indices, distance bits and canaries of one row of the table, with and without a distance buffer"""
    X, U = K.data(case)
    oi, od = K.reference(case)
    idx, bits = run_twice(L, case, X, U)
    np.testing.assert_array_equal(idx, oi)
    np.testing.assert_array_equal(bits, od.view(np.uint64))


@pytest.mark.parametrize("case", K.NAN_CASES, ids=K.case_id)
def test_nan_rows_get_valid_indices_and_disturb_nobody(L, case):
    """The device entry cannot refuse bad input, but every later stage uses the indices as addresses: rows 0, 37 and n - 1 of
    X all NaN (the last one is also what the lanes past n clamp to) get indices in [0, s) from every family's own sentinel
    handling -- the list that never fills, the running minimum that never moves, the screen's rescan that finds nothing -- and
    every other row is the oracle's on the clean input, bit for bit"""
    X, U = K.data(case)
    oi, od = K.reference(case)
    Xb = X.copy()
    Xb[list(K.NAN_ROWS)] = np.nan
    idx, bits = run_twice(L, case, Xb, U)
    assert idx.min() >= 0 and idx.max() < case.s
    clean = np.setdiff1d(np.arange(case.n), K.NAN_ROWS)
    np.testing.assert_array_equal(idx[clean], oi[clean])
    np.testing.assert_array_equal(bits[clean], od.view(np.uint64)[clean])


REFUSALS = [("r = 0", dict(r=0), "1 <= r <= s"), ("r = 33", dict(r=33), "exceeds the built maximum"),
            ("r = s + 1", dict(r=41), "1 <= r <= s"), ("ldx = n - 1", dict(ldx=9), "leading dimensions"),
            ("ldo = n - 1", dict(ldo=9), "leading dimensions"), ("d = 0", dict(d=0), "1 <= d <="),
            ("d = FLGP_DMAX + 1", dict(d=K.DMAX + 1), "1 <= d <=")]


@pytest.mark.parametrize("name,over,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_write_nothing(L, name, over, message):
    """FLGP_ERR_INVALID with a message, before anything is launched: both outputs all canary"""
    case = K.Case(10, 3, 40, 2, {}, "mixture")
    X, U = K.data(case)
    pl = placed(L, X, U, case.r)
    rc = knn(L, pl, **over)
    assert rc == FLGP_ERR_INVALID and message in L.flgp_last_error().decode()
    assert pl.idx_untouched(whole=True) and pl.dist_untouched(whole=True)
    _lib.check(knn(L, pl))                  # and the same buffers serve the valid call
    idx, bits = pl.read()
    oi, od = K.reference(case)
    np.testing.assert_array_equal(idx, oi)
    np.testing.assert_array_equal(bits, od.view(np.uint64))


@pytest.mark.parametrize("d,r", [(3, 2), (3, 1), (40, 5), (70, 5)], ids=lambda v: str(v))
def test_no_points_is_ok_and_writes_nothing(L, d, r):
    case = K.Case(10, d, 40, r, {}, "mixture")
    X, U = K.data(case)
    pl = placed(L, X, U, r)
    assert knn(L, pl, n=0) == FLGP_OK
    assert pl.idx_untouched(whole=True) and pl.dist_untouched(whole=True)
