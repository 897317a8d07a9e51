"""GPU: the regression training objective against the pinned bits of tests/golden/regression_objective_bits.npz.

flgp_eigenpair_regression_objective is the batch of one: it and flgp_regression_batch_eval run the same Woodbury launches
and the same direct steps.  The fixture holds what the single entry returned on an MI355X while it still
ran steps of its own -- an independent implementation -- for every case of regression_objective_cases.CASES
(tests/golden/record_regression_objective_bits.py).  Both entries have to return exactly those value and gradient bits,
and the recorded outcome of the two failure cases.  No tolerance appears in this file."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regression_objective_cases as C  # noqa: E402
from flgp_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pairs():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()
    made = C.synthetic_pairs()
    yield made
    for _, _, rp in made:
        rp.free()


@pytest.fixture(scope="module")
def pinned():
    return C.load_bits()


def same_bits(got, want):
    """got: (value, value-only value, gradient); want: their pinned uint64 patterns"""
    v, v0, g = got
    assert C.bits(v)[0] == want[0] and C.bits(v0)[0] == want[1], (v, v0, np.array(want[:2], dtype=np.uint64).view(np.float64))
    assert np.array_equal(C.bits(g), want[2]), (g, want[2].view(np.float64))


@pytest.mark.parametrize("c", C.CASES, ids=lambda c: c.key)
def test_both_entries_return_the_pinned_bits(pairs, pinned, c):
    vb, v0b, gb, code, _ = pinned[c.key]
    assert code == 0 and gb.size == (c.m + 1 if c.noise == "different" else 2)
    want = (vb, v0b, gb)
    same_bits(C.run_single(pairs, c), want)
    same_bits(C.run_batch(pairs, c, B=1), want)
    same_bits(C.run_batch(pairs, c, B=3), want)


@pytest.mark.parametrize("f", C.FAILURES, ids=lambda f: f.key)
def test_the_failure_cases_reproduce_their_outcome(pinned, f):
    vb, v0b, gb, code, message = pinned[f.key]
    got = C.run_failure(f)
    assert (got[0], got[1]) == (code, message)
    viab = C.run_failure(f, batch=True)
    assert viab[0] == code
    if code:
        head = "regression_objective: "
        assert message.startswith(head)
        assert viab[1] == "position 0: regression_objective_batch: " + message[len(head):]
    else:
        for r in (got, viab):
            same_bits(r[2:], (vb, v0b, gb))


@pytest.mark.parametrize("noise", ["same", "different"])
def test_a_range_read_in_place_at_an_odd_row_of_an_odd_n(pairs, noise):
    """A context of one pair reads a range of rows where the pair keeps them: base vectors + row0 at the leading dimension n.
    Row 101 of a pair with n = 3001: the base is not 16-byte aligned and the stride is odd (the GEMM's general loads).  The
    same problem in a context that lists a second pair reads a gathered copy at ld = m -- the route the fixture pins on its
    ranges -- so the bits have to be equal."""
    from flgp_amd import api
    n, K, m, q = 3001, 65, 300, 3
    made = []
    for seed in (41, 42):
        values, V = C.R.synthetic_pair(n, K, np.random.default_rng(seed))
        made.append(api.ResidentEigenPair.from_host(api.EigenPair(values, V)))
    rng = np.random.default_rng(43)
    idx = np.arange(101, 101 + m)
    Y = rng.standard_normal((m, q))
    x = np.r_[1.7, 0.3] if noise == "same" else np.r_[1.7, rng.uniform(0.05, 0.4, m)]
    kw = dict(sigma=C.SIGMA, noise=noise, approach="posterior")
    two = api.RegressionObjectiveBatch(made, K, idx, Y, **kw)
    one = api.RegressionObjectiveBatch(made[:1], K, idx, Y, **kw)
    try:
        prob = np.zeros(1, dtype=np.int32)
        v, g = two(x[None, :], prob=prob)
        want = (C.bits(v)[0], C.bits(two(x[None, :], prob=prob, grad=False))[0], C.bits(g))
        v, g = one(x[None, :])
        same_bits((v[0], one(x[None, :], grad=False)[0], g[0]), want)
        v, g = made[0].regression_objective(x, K, idx, Y, **kw)
        same_bits((v, made[0].regression_objective(x, K, idx, Y, grad=False, **kw), g), want)
    finally:
        two.free(); one.free()
        for rp in made:
            rp.free()


def prof_count(name):
    c = ctypes.c_int(); ms = ctypes.c_double(); w = ctypes.c_double()
    _lib.lib().flgp_prof_query(name.encode(), ctypes.addressof(c), ctypes.addressof(ms), ctypes.addressof(w))
    return c.value


@pytest.mark.parametrize("K,m,batched,single", [(200, 201, 1, 0), (200, 200, 0, 1)], ids=["woodbury", "direct"])
def test_the_single_entry_runs_the_batch_launches(pairs, K, m, batched, single):
    """m > K: the chunk's blocked Cholesky, once; m <= K: the pool item's own factorisation, once"""
    c = next(c for c in C.CASES if (c.K, c.m) == (K, m))
    idx, Y, x = C.inputs(c)
    L = _lib.lib()
    L.flgp_prof_reset(); L.flgp_prof_enable(2)
    try:
        pairs[c.pair][2].regression_objective(x, K, idx, Y, sigma=C.SIGMA, noise=c.noise, approach=c.approach)
    finally:
        L.flgp_prof_enable(0)
    assert prof_count("chol_blocked_batch") == batched
    assert prof_count("chol_blocked") == single
    L.flgp_prof_reset()
