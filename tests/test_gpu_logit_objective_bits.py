"""GPU: the logit training objective against the pinned bits of tests/golden/logit_objective_bits.npz.

flgp_eigenpair_logit_objective is the batch of one: it and flgp_eigenpair_logit_objective_batch run the same Newton loops
(DESIGN 8 f-15).  The fixture holds what the single entry returned on an MI355X while it still ran loops of its own -- an
independent implementation -- for every case of logit_objective_cases.GROUPS (tests/golden/record_logit_objective_bits.py).
Both entries have to return exactly those value bits and iteration counts.  No tolerance appears in this file."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logit_objective_cases as C  # noqa: E402
from flgp_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pair():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does (as the parity suite's
    fixtures do), or torch finds no GPU for the rest of the process."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()
    _, rp = C.synthetic_pair(C.N_ROWS, C.N_COLS, C.PAIR_SEED)
    yield rp
    rp.free()


@pytest.fixture(scope="module")
def pinned():
    return C.load_bits()


def same_bits(got, bits, iters):
    gv, gi = got
    assert np.array_equal(gi, iters), (gi, iters)
    assert np.array_equal(np.asarray(gv, dtype=np.float64).view(np.uint64), bits), (gv, bits.view(np.float64))


@pytest.mark.parametrize("g", C.GROUPS, ids=lambda g: g.key)
def test_both_entries_return_the_pinned_bits(pair, pinned, g):
    bits, iters = pinned[g.key]
    if g.max_iter == 2:
        assert (iters == 2).all()                                 # the case is there for the cap
    same_bits(C.run_single(pair, g), bits, iters)
    idx, Y, N, kw = C.group_inputs(g)
    cols, ts = C.problems(g)
    same_bits(pair.logit_objective_batch(ts, g.K, idx, Y, col=cols, N=N, return_iters=True, **kw), bits, iters)


def prof_count(name):
    c = ctypes.c_int(); ms = ctypes.c_double(); w = ctypes.c_double()
    _lib.lib().flgp_prof_query(name.encode(), ctypes.addressof(c), ctypes.addressof(ms), ctypes.addressof(w))
    return c.value


def test_the_single_entry_runs_the_batch_loop(pair):
    g = next(g for g in C.GROUPS if (g.K, g.m) == (200, 201))
    idx, Y, N, kw = C.group_inputs(g)
    L = _lib.lib()
    L.flgp_prof_reset(); L.flgp_prof_enable(2)
    try:
        _, its = pair.logit_objective(C.TS[0], g.K, idx, Y[:, 0], N=N, return_iters=True, **kw)
    finally:
        L.flgp_prof_enable(0)
    assert its >= 2
    assert prof_count("logit_lr_batch_iter") == its
    assert prof_count("logit_lr_newton_iter") == 0
    L.flgp_prof_reset()
