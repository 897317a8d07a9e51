"""GPU: the Polya-Gamma prediction against the pinned bits of tests/golden/pg_predict_bits.npz.

flgp_eigenpair_pg_predict is the batch of one and flgp_eigenpair_pg_predict_multiclass the batch of J on the indicator
matrix: the three resident-pair entries run the same chains.  The fixture holds what the binary and the
one-vs-rest entry returned on an MI355X while they still ran a Woodbury sweep of their own, one chain after another -- an
independent implementation -- for every case of pg_predict_cases.CASES (tests/golden/record_pg_predict_bits.py).  Every
entry has to return exactly those bits.  No tolerance appears in this file."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pg_predict_cases as C  # noqa: E402
from flgp_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pairs():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()
    made = C.Pairs()
    yield made
    made.free()


@pytest.fixture(scope="module")
def pinned():
    return C.load_bits()


def same_bits(c, got, want, what):
    for k in C.out_keys(c):
        assert got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(C.bits(got[k]), want[k]), (what, k)


@pytest.mark.parametrize("c", [c for c in C.CASES if c.entry == "binary"], ids=lambda c: c.key)
def test_the_binary_and_the_batch_entry_return_the_pinned_bits(pairs, pinned, c):
    rp = pairs(c)
    same_bits(c, C.run_binary(rp, c), pinned[c.key], "binary")
    for mp in (0, 1):
        same_bits(c, C.run_batch(rp, c, mp), pinned[c.key], f"batch, max_parallel={mp}")


@pytest.mark.parametrize("c", [c for c in C.CASES if c.entry == "classes"], ids=lambda c: c.key)
def test_the_one_vs_rest_and_the_batch_entry_return_the_pinned_bits(pairs, pinned, c):
    rp = pairs(c)
    same_bits(c, C.run_classes(rp, c), pinned[c.key], "classes")
    for mp in (0, 1, 3):
        same_bits(c, C.run_classes_batch(rp, c, mp), pinned[c.key], f"batch, max_parallel={mp}")


def prof_count(name):
    c = ctypes.c_int(); ms = ctypes.c_double(); w = ctypes.c_double()
    _lib.lib().flgp_prof_query(name.encode(), ctypes.addressof(c), ctypes.addressof(ms), ctypes.addressof(w))
    return c.value


def counted(call):
    """(pg_batch_sweep, pg_sweep) scopes entered by call()"""
    L = _lib.lib()
    L.flgp_prof_reset(); L.flgp_prof_enable(2)
    try:
        call()
    finally:
        L.flgp_prof_enable(0)
    counts = prof_count("pg_batch_sweep"), prof_count("pg_sweep")
    L.flgp_prof_reset()
    return counts


def test_the_other_entries_run_the_batch_loop(pairs):
    by_key = {c.key: c for c in C.CASES}

    def one_binary_call(c):
        idx0, idx1 = C.rows(c)
        return lambda: pairs(c).test_pgbinary(idx0, idx1, c.K, c.ts[0], C.responses(c)[:, 0], C.SIGMA, c.sigma_nv,
                                              N_sample=C.N_SAMPLE, seed=c.seed[0])

    c = by_key["binary-K16-m48-nv1"]                              # m > K: the batched sweep, once per sample
    assert counted(one_binary_call(c)) == (C.N_SAMPLE, 0)
    c = by_key["classes-K12-m60-J3"]                              # the J classes share every sweep: not J N_sample
    assert len(c.ts) == 3
    assert counted(lambda: C.run_classes(pairs(c), c)) == (C.N_SAMPLE, 0)
    c = by_key["binary-K40-m24-nv1"]                              # m <= K: a pool worker on the m x m route
    assert counted(one_binary_call(c)) == (0, C.N_SAMPLE)
