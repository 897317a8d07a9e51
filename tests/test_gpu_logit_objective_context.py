"""GPU: the logit training context (flgp_logit_batch_*, LogitObjectiveBatch): B (pair, labels, t) problems per
evaluation on state made once.  The contract is equality of bits with the single entry flgp_eigenpair_logit_objective on
the position's pair, column and t -- for any B, P, A, order, repeats and chunk size, whatever shares the evaluation and
whatever the context evaluated before.  The independent reference is tests/golden/logit_objective_bits.npz (the bits of the
loop the single entry ran before it became the batch of one), which a context on the seed-21 pair reproduces group by
group.  No tolerance appears anywhere in this file."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flgp_amd import _lib, api  # noqa: E402
from logit_objective_cases import (DENSE_SHAPES, GROUPS, LOWRANK_SHAPES, PRIOR, TS, group_inputs, load_bits,  # noqa: E402
                                   problems, responses, rows, synthetic_pair)

pytestmark = pytest.mark.gpu

PAIRS = [(21, 3000, 240), (22, 2600, 200), (23, 3100, 210)]            # (seed, n, columns)
N_MIN = min(n for _, n, _ in PAIRS)                                    # rows are drawn below the smallest n
PATTERN = (0, 1, 0, 2, 1)                                              # eps = [a, b, a, c, b, ...]: repeats apart, P != B
WHO = "logit_objective_context"


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does (as the parity suite's
    fixtures do), or torch finds no GPU for the rest of the process."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()


@pytest.fixture(scope="module")
def pairs(torch_first):
    made = [synthetic_pair(n, k, seed=seed)[1] for seed, n, k in PAIRS]
    yield made
    for rp in made:
        rp.free()


@pytest.fixture(scope="module")
def pinned():
    return load_bits()


class Single:
    """The reference: the single entry per (pair, column, t) of one configuration, each made once and left unchanged."""

    def __init__(self, rps, K, idx, Y, N, sigma, approach, prior, max_iter=100):
        self.rps, self.K, self.idx, self.Y, self.N = rps, K, idx, Y, N
        self.kw = dict(sigma=sigma, approach=approach, prior=prior, max_iter=max_iter)
        self.done = {}

    def __call__(self, pair_of, cols, ts):
        vals, its = [], []
        for p, c, t in zip(pair_of, cols, ts):
            key = (int(p), int(c), float(t))
            if key not in self.done:
                self.done[key] = self.rps[int(p)].logit_objective(float(t), self.K, self.idx, self.Y[:, int(c)], N=self.N,
                                                                  return_iters=True, **self.kw)
            vals.append(self.done[key][0]); its.append(self.done[key][1])
        return np.array(vals, dtype=np.float64), np.array(its, dtype=np.int32)

    def context(self, pair_of, cols, max_parallel=0):
        return api.LogitObjectiveBatch([self.rps[int(p)] for p in pair_of], self.K, self.idx, self.Y, col=cols, N=self.N,
                                       max_parallel=max_parallel, **self.kw)


def same_bits(got, ref):
    (gv, gi), (rv, ri) = got, ref
    assert np.array_equal(gi, ri), (gi, ri)
    assert gv.tobytes() == rv.tobytes(), (gv, rv)


def configurations(rps, K, m, kinds=("perm", "repeated"), max_iter=100):
    """the two configurations of the batch tests on rows below the smallest n: the indicators under N = NULL and
    "marginal", all six columns under the binomial N and "posterior" with PRIOR"""
    _, Y, N = responses(m, 7 * K + m)
    return [Single(rps, K, rows(N_MIN, m, kinds[0], 31 * K + m), Y[:, :5], None, 1e-3, "marginal", None, max_iter),
            Single(rps, K, rows(N_MIN, m, kinds[1], 37 * K + m), Y, N, 0.1, "posterior", PRIOR, max_iter)]


def pattern(B):
    return np.array([PATTERN[b % len(PATTERN)] for b in range(B)])


# ---- 1. the pinned bits: a context on the seed-21 pair alone, one evaluation per group --------------------------------------
@pytest.mark.parametrize("g", GROUPS, ids=[g.key for g in GROUPS])
def test_a_context_reproduces_the_pinned_bits(pairs, pinned, g):
    idx, Y, N, kw = group_inputs(g)
    cols, ts = problems(g)
    ctx = api.LogitObjectiveBatch([pairs[0]] * len(cols), g.K, idx, Y, col=cols, N=N, **kw)
    try:
        assert (ctx.B, ctx.P) == (len(cols), 1)
        values, its = ctx(ts, return_iters=True)
    finally:
        ctx.free()
    bits, ref_its = pinned[g.key]
    assert np.array_equal(its, ref_its), (its, ref_its)
    assert np.array_equal(values.view(np.uint64), bits), (values, bits.view(np.float64))


# ---- 2. several pairs against the single entry ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K,m", LOWRANK_SHAPES + DENSE_SHAPES)
def test_several_pairs_are_the_single_entry_on_each(pairs, K, m):
    rng = np.random.default_rng(K + m)
    for S in configurations(pairs, K, m):
        ncols = S.Y.shape[1]
        # the precondition: at a fixed (column, t) the pairs differ, or a context that read the wrong pair would pass
        v, _ = S([0, 1, 2], [0, 0, 0], [1.0, 1.0, 1.0])
        assert len({x.tobytes() for x in v}) >= 2, v
        for B in (1, 2, 7, 33):
            pair_of = pattern(B)
            cols = rng.integers(0, ncols, B).astype(np.int32)
            ts = np.array(TS)[rng.integers(0, len(TS), B)]
            ctx = S.context(pair_of, cols, max_parallel=3 if m <= K and B > 2 else 0)
            try:
                assert (ctx.B, ctx.P) == (B, len(set(pair_of.tolist())))
                same_bits(ctx(ts, return_iters=True), S(pair_of, cols, ts))
            finally:
                ctx.free()


# ---- 3. slots leave at different times across pairs ----------------------------------------------------------------------------
@pytest.mark.parametrize("K,m", [(200, 201), (200, 1000)])
def test_slots_leave_at_different_iterations_across_pairs(pairs, K, m):
    idx = rows(N_MIN, m, "perm", 41 * K + m)
    _, Y, _ = responses(m, 43 * K + m, singleton=False)
    ts = np.tile(np.repeat(np.array(TS), 5), 3)                        # TS x five columns x three pairs
    cols = np.tile(np.arange(5, dtype=np.int32), 4 * 3)
    pair_of = np.arange(60) % 3                                          # neighbours in the chunk sit on different pairs
    for max_iter in (100, 2):
        S = Single(pairs, K, idx, Y[:, :5], None, 1e-3, "marginal", None, max_iter=max_iter)
        ref = S(pair_of, cols, ts)
        if max_iter == 100:
            assert len(set(ref[1].tolist())) >= 2, ref[1]                # the precondition: the chunk does see slots leave
        else:
            assert (ref[1] == 2).all()
        ctx = S.context(pair_of, cols, max_parallel=60)
        try:
            assert ctx.chunk == 60
            same_bits(ctx(ts, return_iters=True), ref)
        finally:
            ctx.free()


# ---- 4. chunks, order, company, history ----------------------------------------------------------------------------------------
def test_chunks_order_company_and_history_do_not_matter(pairs):
    K, m = 200, 201
    idx = rows(N_MIN, m, "perm", 51)
    _, Y, N = responses(m, 52)
    S = Single(pairs, K, idx, Y, N, 1e-3, "posterior", None)
    rng = np.random.default_rng(53)
    B = 11
    pair_of = pattern(B)
    cols = rng.integers(0, 6, B).astype(np.int32)
    ts = np.array(TS)[rng.integers(0, len(TS), B)]
    ts[0], ts[1] = 0.3, 20.0                                           # two iteration counts at this shape
    ref = S(pair_of, cols, ts)
    for mp in (1, 3, 0):
        ctx = S.context(pair_of, cols, max_parallel=mp)
        try:
            assert ctx.chunk == (mp if mp else B)
            same_bits(ctx(ts, return_iters=True), ref)
            # prob as a permutation, a subset and with repeats: every position its problem's bits at its own t
            for prob in (rng.permutation(B), np.sort(rng.choice(B, 4, replace=False))[::-1], rng.integers(0, B, 17)):
                prob = np.ascontiguousarray(prob, dtype=np.int32)
                t2 = np.array(TS)[rng.integers(0, len(TS), prob.size)]
                same_bits(ctx(t2, prob=prob, return_iters=True), S(pair_of[prob], cols[prob], t2))
            # history: the first arguments again return the first bits
            same_bits(ctx(ts, return_iters=True), ref)
        finally:
            ctx.free()


# ---- 5. rows in place and gathered -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,m", [(64, 65), (200, 201), (50, 40)])
def test_a_range_of_rows_in_place_and_gathered(pairs, K, m):
    idx = np.arange(37, 37 + m, dtype=np.int32)                        # an odd first row
    _, Y, N = responses(m, 7 * K + m)
    S = Single(pairs, K, idx, Y, N, 1e-3, "posterior", PRIOR)
    rng = np.random.default_rng(55)
    for pair_of in (np.array([1, 1, 1, 1, 1]), np.array([0, 1, 0, 2, 1])):
        cols = rng.integers(0, 6, 5).astype(np.int32)
        ts = np.array(TS)[rng.integers(0, len(TS), 5)]
        ctx = S.context(pair_of, cols)
        try:
            same_bits(ctx(ts, return_iters=True), S(pair_of, cols, ts))
        finally:
            ctx.free()


# ---- 6. status, and refusals on a live handle ------------------------------------------------------------------------------------
def raw_eval(ctx, prob, ts, status=False):
    ts = np.ascontiguousarray(ts, dtype=np.float64)
    prob = None if prob is None else np.ascontiguousarray(prob, dtype=np.int32)
    values = np.zeros(ts.size); its = np.zeros(ts.size, dtype=np.int32)
    stat = np.full(ts.size, 99, dtype=np.int32) if status else None
    rc = _lib.lib().flgp_logit_batch_eval(ctx._h, None if prob is None else prob.ctypes.data, ts.size, ts.ctypes.data,
                                          values.ctypes.data, its.ctypes.data, None if stat is None else stat.ctypes.data)
    return rc, values, its, stat


@pytest.mark.parametrize("K,m", [(64, 65), (50, 40)])
def test_status_and_refusals_leave_the_handle_usable(pairs, K, m):
    idx = rows(N_MIN, m, "perm", 91)
    _, Y, _ = responses(m, 92)
    S = Single(pairs, K, idx, Y[:, :5], None, 1e-3, "posterior", None)
    pair_of = pattern(5)
    cols = np.arange(5, dtype=np.int32)
    ts = np.array([0.3, 1.0, 4.0, 20.0, 1.0])
    ref = S(pair_of, cols, ts)
    L = _lib.lib()
    ctx = S.context(pair_of, cols)
    try:
        values, its, status = ctx(ts, return_iters=True, return_status=True)
        assert (status == 0).all()
        same_bits((values, its), ref)
        same_bits(ctx(ts, return_iters=True), ref)
        rc, _, _, _ = raw_eval(ctx, [0, 1, 5, 3, 4], ts)
        assert rc == -1
        assert L.flgp_last_error().decode() == "position 2 (t=4): %s: prob=5 is outside [0, B=5)" % WHO
        with pytest.raises(api.FlgpError) as e:                        # the wrapper's own refusal: the same text
            ctx(ts, prob=[0, 1, 5, 3, 4])
        assert e.value.code == -1 and e.value.message == L.flgp_last_error().decode()
        tn = ts.copy(); tn[3] = np.inf
        rc, _, _, _ = raw_eval(ctx, None, tn, status=True)
        assert rc == -1
        assert L.flgp_last_error().decode() == "position 3 (t=inf): %s: t must be finite" % WHO
        with pytest.raises(api.FlgpError) as e:
            ctx(tn)
        assert e.value.message == L.flgp_last_error().decode()
        tz = ts.copy(); tz[4] = 0.0
        rc, _, _, _ = raw_eval(ctx, None, tz)
        assert rc == -1
        assert L.flgp_last_error().decode() == 'position 4 (t=0): %s: t must be positive under "posterior"' % WHO
        assert raw_eval(ctx, None, ts[:4])[0] == -1                     # prob NULL with A != B
        assert L.flgp_last_error().decode() == "%s: prob may be NULL only if A == B (A=4, B=5)" % WHO
        # the next evaluation gives the reference bits, with and without the status array
        rc, v1, i1, s1 = raw_eval(ctx, None, ts, status=True)
        assert rc == 0 and (s1 == 0).all()
        same_bits((v1, i1), ref)
        rc, v2, i2, _ = raw_eval(ctx, None, ts)
        assert rc == 0
        same_bits((v2, i2), ref)
    finally:
        ctx.free()


def test_create_names_the_problem_it_refuses(pairs):
    K, m = 64, 65
    idx = rows(N_MIN, m, "perm", 93)
    _, Y, _ = responses(m, 94)
    Y = Y[:, :5]
    a, b, c = pairs
    with pytest.raises(api.FlgpError) as e:                            # K above the second pair's own (200 columns)
        api.LogitObjectiveBatch([a, c, b], 205, idx, Y, col=[0, 1, 2])
    assert e.value.code == -1 and e.value.message.startswith("problem 2: %s: bad shape (K=205 of 200" % WHO)
    with pytest.raises(api.FlgpError) as e:                            # a row the second pair does not have
        api.LogitObjectiveBatch([a, b, c], K, np.r_[idx[:-1], 2600], Y, col=[0, 1, 2])
    assert e.value.message == "problem 1: %s: idx[64]=2600 out of range" % WHO
    with pytest.raises(api.FlgpError) as e:
        api.LogitObjectiveBatch([a, b, c], K, idx, Y, col=[0, 5, 2])
    assert e.value.message == "problem 1: %s: col=5 is outside [0, ncol=5)" % WHO
    with pytest.raises(api.FlgpError) as e:
        api.LogitObjectiveBatch([a, b, c], K, idx, Y)                   # col None with ncol != B
    assert e.value.message == "%s: col may be NULL only if ncol == B (ncol=5, B=3)" % WHO
    ctx = api.LogitObjectiveBatch([a, b, a, c, b], K, idx, Y)           # col None: problem b is column b
    try:
        B, P, Kc, mc, ncol, chunk = (np.zeros(1, dtype=np.int32) for _ in range(6))
        assert _lib.lib().flgp_logit_batch_dims(ctx._h, *(x.ctypes.data for x in (B, P, Kc, mc, ncol, chunk))) == 0
        assert [int(x[0]) for x in (B, P, Kc, mc, ncol, chunk)] == [5, 3, K, m, 5, 5]
    finally:
        ctx.free()


# ---- 7. the one-vs-rest grid ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,m", [(64, 65), (50, 40)])
def test_for_classes_is_the_multiclass_entry_on_each_pair(pairs, K, m):
    idx = rows(N_MIN, m, "perm", 81)
    labels, _, _ = responses(m, 82)
    two = [pairs[2], pairs[1]]
    ts = np.array([[0.3, 1.0, 4.0, 20.0, 1.0], [20.0, 0.3, 1.0, 4.0, 4.0]])
    ctx = api.LogitObjectiveBatch.for_classes(two, K, idx, labels, sigma=1e-3, approach="posterior", prior=PRIOR)
    try:
        assert (ctx.B, ctx.P, ctx.J) == (10, 2, 5)
        gv, gi = ctx(ts.reshape(-1), return_iters=True)
    finally:
        ctx.free()
    for p, rp in enumerate(two):
        rv, ri = rp.logit_objective_multiclass(ts[p], K, idx, labels, sigma=1e-3, approach="posterior", prior=PRIOR,
                                               return_iters=True)
        same_bits((gv[5 * p:5 * p + 5], gi[5 * p:5 * p + 5]), (rv, ri))
