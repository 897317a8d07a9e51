"""GPU: the logit posterior against the pinned bits of tests/golden/logit_posterior_bits.npz.

flgp_eigenpair_logit_posterior is the batch of one and the one-vs-rest entries are the batch of J on the indicator matrix:
the three run the same Newton loop.  The fixture holds what the binary entry and the one-vs-rest entry
returned on an MI355X while each still ran loops of its own -- independent implementations -- for every case of
logit_posterior_cases.CASES (tests/golden/record_logit_posterior_bits.py).  Every entry has to return exactly those bits of
mean and cov, those iteration counts and, for the refused cases, that status and text.  No tolerance appears in this file."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logit_posterior_cases as C  # noqa: E402
from flgp_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pairs():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does (as the parity suite's
    fixtures do), or torch finds no GPU for the rest of the process."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()
    made = C.Pairs()
    yield made
    made.free()


@pytest.fixture(scope="module")
def pinned():
    return C.load_bits()


def same_bits(got, want, what):
    mean, cov, its, code, message = got
    assert (code, message) == (want.code, want.message), what
    assert np.array_equal(its, want.iters), (what, its, want.iters)
    assert mean.shape == want.mean.shape and cov.shape == want.cov.shape, what
    assert np.array_equal(np.ascontiguousarray(mean).view(np.uint64), want.mean), (what, "mean")
    assert np.array_equal(np.ascontiguousarray(cov).view(np.uint64), want.cov), (what, "cov")


def batch_text(c, message):
    """The batch entry's wording of a refusal the binary entry words as `message`."""
    return "problem 0 (t=%g): " % c.ts[0] + message.replace("logit_posterior:", "logit_posterior_batch:")


@pytest.mark.parametrize("c", [c for c in C.CASES if c.entry == "binary"], ids=lambda c: c.key)
def test_the_binary_and_the_batch_entry_return_the_pinned_bits(pairs, pinned, c):
    want = pinned[c.key]
    rp = pairs(c)
    if c.max_iter == 2:
        assert (want.iters == 2).all()                            # the case is there for the cap
    same_bits(C.run_binary(rp, c), want, "binary")
    if c.fails:
        want = want._replace(message=batch_text(c, want.message))
    for mp in (0, 1):
        same_bits(C.run_batch(rp, c, mp), want, f"batch, max_parallel={mp}")


@pytest.mark.parametrize("c", [c for c in C.CASES if c.entry == "classes"], ids=lambda c: c.key)
def test_the_one_vs_rest_and_the_batch_entry_return_the_pinned_bits(pairs, pinned, c):
    want = pinned[c.key]
    rp = pairs(c)
    for mp in (1, 3, 0):
        same_bits(C.run_classes(rp, c, mp), want, f"classes, max_parallel={mp}")
    if c.fails:
        assert want.code == -5 and want.message.startswith("logit_posterior_multiclass: class 0: ")
        want = want._replace(message=batch_text(c, want.message.replace("logit_posterior_multiclass: class 0:", "logit_posterior:")))
    for mp in (0, 1):
        same_bits(C.run_batch(rp, c, mp), want, f"batch, max_parallel={mp}")


def prof_count(name):
    c = ctypes.c_int(); ms = ctypes.c_double(); w = ctypes.c_double()
    _lib.lib().flgp_prof_query(name.encode(), ctypes.addressof(c), ctypes.addressof(ms), ctypes.addressof(w))
    return c.value


def test_the_other_entries_run_the_batch_loop(pairs):
    c = next(c for c in C.CASES if c.key == "binary-mixed-K16-m48-maxiter100")
    rp = pairs(c)
    idx0, idx1, Y = C.case_inputs(c)
    L = _lib.lib()
    L.flgp_prof_reset(); L.flgp_prof_enable(2)
    try:
        _, its = rp.logit_posterior(idx0, idx1, c.K, c.ts[2], Y[:, c.cols[2]], c.sig[0], c.sig[1], tol=C.TOL, return_iters=True)
    finally:
        L.flgp_prof_enable(0)
    assert its >= 2
    assert prof_count("logit_ws_batch_iter") == its
    assert prof_count("logit_ws_newton_iter") == 0
    J = 4
    labels = (np.arange(c.m) % J).astype(np.float64)
    L.flgp_prof_reset(); L.flgp_prof_enable(2)
    try:
        _, its = rp.logit_posterior_multiclass(idx0, idx1, c.K, [0.3, 12.0, 200.0, 8.0], labels, c.sig[1], sigma11=c.sig[0],
                                               tol=C.TOL, max_parallel=J, return_iters=True)
    finally:
        L.flgp_prof_enable(0)
    assert prof_count("logit_ws_batch_iter") == its.max() < its.sum()
    assert prof_count("logit_ws_newton_iter") == 0
    assert prof_count("gpc_predict_rows_multi") == 1
    L.flgp_prof_reset()
