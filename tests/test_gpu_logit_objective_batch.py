"""GPU: the logit training objective for B problems in one call (flgp_eigenpair_logit_objective_batch).
The single entry flgp_eigenpair_logit_objective is the reference and the contract is equality of bits: every value and
every iteration count of a batch is what the single entry returns for that column at that t -- for any B, any order, any
chunk size and whichever other problems share the call.  The single entry is now the batch of one, so that reference
shares the batch's code: what it shows here is that a problem's bits do not depend on its company.  The independent
reference is the pinned bits of the loop the single entry ran before (tests/golden/logit_objective_bits.npz), which
test_gpu_logit_objective_bits.py holds both entries to on the shapes and configurations of this file.  No tolerance
appears anywhere in this file."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flgp_amd import _lib  # noqa: E402
from logit_objective_cases import (LOWRANK_SHAPES, N_COLS, N_ROWS, PRIOR, TS, responses, rows,  # noqa: E402
                                   synthetic_pair)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does (as the parity suite's
    fixtures do), or torch finds no GPU for the rest of the process."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()


@pytest.fixture(scope="module")
def pair(torch_first):
    _, rp = synthetic_pair(N_ROWS, N_COLS, seed=21)
    yield rp
    rp.free()


class Single:
    """The reference: single calls (batches of one), each (column, t) of a configuration made once."""

    def __init__(self, rp, K, idx, Y, N, sigma, approach, prior, max_iter=100):
        self.rp, self.K, self.idx, self.Y, self.N = rp, K, idx, Y, N
        self.kw = dict(sigma=sigma, approach=approach, prior=prior, max_iter=max_iter)
        self.done = {}

    def __call__(self, cols, ts):
        vals, its = [], []
        for c, t in zip(cols, ts):
            key = (int(c), float(t))
            if key not in self.done:
                self.done[key] = self.rp.logit_objective(float(t), self.K, self.idx, self.Y[:, int(c)], N=self.N,
                                                         return_iters=True, **self.kw)
            vals.append(self.done[key][0]); its.append(self.done[key][1])
        return np.array(vals, dtype=np.float64), np.array(its, dtype=np.int32)

    def batch(self, cols, ts, max_parallel=0):
        return self.rp.logit_objective_batch(ts, self.K, self.idx, self.Y, col=cols, N=self.N, max_parallel=max_parallel,
                                             return_iters=True, **self.kw)


def same_bits(got, ref):
    (gv, gi), (rv, ri) = got, ref
    assert np.array_equal(gi, ri), (gi, ri)
    assert gv.tobytes() == rv.tobytes(), (gv, rv)


def draw(rng, B, ncols):
    return rng.integers(0, ncols, B).astype(np.int32), np.array(TS)[rng.integers(0, len(TS), B)]


# ---- 1. bit for bit against the single entry, m > K -------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [1e-3, 0.1])
@pytest.mark.parametrize("kind", ["perm", "repeated"])
@pytest.mark.parametrize("K,m", LOWRANK_SHAPES)
def test_lowrank_batch_is_the_single_entry(pair, K, m, kind, sigma):
    idx = rows(N_ROWS, m, kind, 31 * K + m)
    _, Y, N = responses(m, 7 * K + m)
    rng = np.random.default_rng(K + m)
    configs = [Single(pair, K, idx, Y[:, :5], None, sigma, "marginal", None),      # the one-vs-rest indicators, N = 1
               Single(pair, K, idx, Y, N, sigma, "posterior", PRIOR)]              # binomial N, a prior of the caller's
    for S in configs:
        ncols = S.Y.shape[1]
        for B in (1, 2, 7, 33):
            cols, ts = draw(rng, B, ncols)
            if B == 7:
                cols[:3] = cols[0]                                                  # one column, several problems
            same_bits(S.batch(cols, ts), S(cols, ts))


# ---- 2. problems that stop at different iterations share a chunk ----------------------------------------------------------
@pytest.mark.parametrize("K,m", LOWRANK_SHAPES)
def test_mixed_iteration_counts_in_one_chunk(pair, K, m):
    idx = rows(N_ROWS, m, "perm", 41 * K + m)
    _, Y, _ = responses(m, 43 * K + m, singleton=False)            # labels = rng.integers(0, 5, m)
    S = Single(pair, K, idx, Y[:, :5], None, 1e-3, "marginal", None)
    cols = np.tile(np.arange(5, dtype=np.int32), 4)
    ts = np.repeat(np.array(TS), 5)
    ref = S(cols, ts)
    if (K, m) != (65, 300):
        assert len(set(ref[1].tolist())) >= 2, ref[1]                # the precondition: the chunk does see problems leave
    same_bits(S.batch(cols, ts, max_parallel=len(cols)), ref)
    # the cap: some problems end at max_iter, the call still succeeds
    S2 = Single(pair, K, idx, Y[:, :5], None, 1e-3, "marginal", None, max_iter=2)
    ref2 = S2(cols, ts)
    assert (ref2[1] == 2).all()
    same_bits(S2.batch(cols, ts), ref2)


# ---- 3. independence of company and order ---------------------------------------------------------------------------------
def test_company_and_order_do_not_matter(pair):
    K, m = 200, 201
    idx = rows(N_ROWS, m, "perm", 51)
    _, Y, N = responses(m, 52)
    S = Single(pair, K, idx, Y, N, 1e-3, "posterior", None)
    rng = np.random.default_rng(53)
    cols, ts = draw(rng, 7, 6)
    ts[0], ts[1] = 0.3, 20.0                                       # two iteration counts at this shape
    ref = S(cols, ts)
    for mp in (1, 3, 7):
        same_bits(S.batch(cols, ts, max_parallel=mp), ref)
    p = rng.permutation(7)
    gv, gi = S.batch(cols[p], ts[p])
    same_bits((gv, gi), (ref[0][p], ref[1][p]))
    ocols, ots = draw(rng, 12, 6)                                  # the batch inside a larger one, chunks of 5
    where = np.sort(rng.choice(19, 7, replace=False))
    bc = np.zeros(19, dtype=np.int32); bt = np.zeros(19)
    mask = np.zeros(19, dtype=bool); mask[where] = True
    bc[mask], bt[mask], bc[~mask], bt[~mask] = cols, ts, ocols, ots
    for mp in (0, 5):
        gv, gi = S.batch(bc, bt, max_parallel=mp)
        same_bits((gv[mask], gi[mask]), ref)


# ---- 4. m <= K: the dense loop on the pool's workers ------------------------------------------------------------------------
@pytest.mark.parametrize("max_parallel", [1, 4])
@pytest.mark.parametrize("K,m", [(50, 40), (200, 200), (65, 1)])
def test_dense_batch_is_the_single_entry(pair, K, m, max_parallel):
    idx = rows(N_ROWS, m, "perm", 61 * K + m)
    _, Y, N = responses(m, 62 * K + m)
    rng = np.random.default_rng(63)
    for S in (Single(pair, K, idx, Y[:, :5], None, 1e-3, "marginal", None), Single(pair, K, idx, Y, N, 0.1, "posterior", PRIOR)):
        cols, ts = draw(rng, 6, S.Y.shape[1])
        same_bits(S.batch(cols, ts, max_parallel=max_parallel), S(cols, ts))


# ---- 5. one sequence of launches per iteration ------------------------------------------------------------------------------
def prof_count(name):
    c = ctypes.c_int(); ms = ctypes.c_double(); w = ctypes.c_double()
    _lib.lib().flgp_prof_query(name.encode(), ctypes.addressof(c), ctypes.addressof(ms), ctypes.addressof(w))
    return c.value


def test_an_iteration_is_one_sequence_for_the_whole_chunk(pair):
    K, m = 200, 201
    idx = rows(N_ROWS, m, "perm", 71)
    _, Y, _ = responses(m, 72, singleton=False)
    S = Single(pair, K, idx, Y[:, :5], None, 1e-3, "marginal", None)
    cols = np.array([0, 1, 2, 3, 4, 0, 1, 2], dtype=np.int32)
    ts = np.array([0.3, 1.0, 4.0, 20.0, 0.3, 20.0, 4.0, 1.0])
    L = _lib.lib()
    L.flgp_prof_reset(); L.flgp_prof_enable(2)
    try:
        _, its = S.batch(cols, ts, max_parallel=8)
    finally:
        L.flgp_prof_enable(0)
    assert prof_count("logit_lr_batch_iter") == its.max() < its.sum()
    assert prof_count("logit_lr_newton_iter") == 0
    L.flgp_prof_reset()


# ---- 6. the one-vs-rest wrapper ---------------------------------------------------------------------------------------------
def test_multiclass_wrapper(pair):
    K, m = 64, 65
    idx = rows(N_ROWS, m, "perm", 81)
    labels, Y, _ = responses(m, 82)
    S = Single(pair, K, idx, Y[:, :5], None, 1e-3, "posterior", None)
    ts = np.array([0.3, 1.0, 4.0, 20.0, 1.0])
    got = pair.logit_objective_multiclass(ts, K, idx, labels, return_iters=True)
    assert got[0].shape == (5,)
    same_bits(got, S(np.arange(5), ts))
    prof = np.array([[0.3, 1.0, 4.0], [1.0, 4.0, 20.0], [20.0, 0.3, 1.0], [4.0, 4.0, 0.3], [1.0, 20.0, 4.0]])
    gv, gi = pair.logit_objective_multiclass(prof, K, idx, labels, return_iters=True)
    assert gv.shape == gi.shape == (5, 3)
    rv, ri = S(np.repeat(np.arange(5), 3), prof.reshape(-1))
    same_bits((gv.reshape(-1), gi.reshape(-1)), (rv, ri))


# ---- 7. refusals on a live handle -------------------------------------------------------------------------------------------
def raw_batch(rp, K, idx, Y, cols, ts, approach=b"posterior", max_parallel=0):
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    Y = np.asfortranarray(Y, dtype=np.float64)
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    ts = np.ascontiguousarray(ts, dtype=np.float64)
    values = np.zeros(ts.size); its = np.zeros(ts.size, dtype=np.int32)
    rc = _lib.lib().flgp_eigenpair_logit_objective_batch(rp._h, K, idx.ctypes.data, idx.size, Y.ctypes.data, Y.shape[1], None,
                                                         cols.ctypes.data, ts.ctypes.data, ts.size, 1e-3, approach, None, 1e-5,
                                                         100, max_parallel, values.ctypes.data, its.ctypes.data)
    return rc, values, its


def test_refusals_name_the_problem_and_leave_the_handle_usable(pair):
    K, m = 64, 65
    idx = rows(N_ROWS, m, "perm", 91)
    _, Y, _ = responses(m, 92)
    Y = Y[:, :5]
    cols = np.array([0, 1, 2, 3, 4], dtype=np.int32)
    ts = np.array([0.3, 1.0, 4.0, 20.0, 1.0])
    L = _lib.lib()
    bad = cols.copy(); bad[3] = 5
    rc, _, _ = raw_batch(pair, K, idx, Y, bad, ts)
    assert rc == -1
    assert L.flgp_last_error().decode() == "problem 3 (t=20): logit_objective_batch: col=5 is outside [0, ncol=5)"
    with pytest.raises(_lib.FlgpError) as e:                       # the wrapper's own refusal: the same text
        pair.logit_objective_batch(ts, K, idx, Y, col=bad)
    assert e.value.code == -1 and e.value.message == L.flgp_last_error().decode()
    tn = ts.copy(); tn[2] = np.nan
    rc, _, _ = raw_batch(pair, K, idx, Y, cols, tn)
    assert rc == -1
    assert L.flgp_last_error().decode() == "problem 2 (t=nan): logit_objective_batch: t must be finite"
    with pytest.raises(_lib.FlgpError) as e:
        pair.logit_objective_batch(tn, K, idx, Y, col=cols)
    assert e.value.message == L.flgp_last_error().decode()
    tz = ts.copy(); tz[4] = 0.0
    rc, _, _ = raw_batch(pair, K, idx, Y, cols, tz)
    assert rc == -1
    assert L.flgp_last_error().decode() == 'problem 4 (t=0): logit_objective_batch: t must be positive under "posterior"'
    # a valid call afterwards: the single entry's bits, twice
    S = Single(pair, K, idx, Y, None, 1e-3, "posterior", None)
    ref = S(cols, ts)
    rc, v1, i1 = raw_batch(pair, K, idx, Y, cols, ts)
    assert rc == 0
    same_bits((v1, i1), ref)
    rc, v2, i2 = raw_batch(pair, K, idx, Y, cols, ts)
    assert rc == 0
    same_bits((v2, i2), (v1, i1))
