"""GPU: the logit posterior for a batch of (labels, t) problems in one call (DESIGN 8 f-17,
flgp_eigenpair_logit_posterior_batch).  The contract is bit for bit: column b of mean / cov and iters[b] are the bytes of the
binary entry flgp_eigenpair_logit_posterior on column col[b] of Y at ts[b] -- on both sides of m = K, for ranges and index
sets, for any B, order, mix, duplicates and chunk size.  Every comparison with the single entry is np.array_equal; one
independent anchor against the dense numpy restatement (tests/np_logit_posterior.py) under its existing tolerances.

The binary entry is the batch of one and the one-vs-rest entry the batch of J (one body in the library), so the
comparisons with them here are consistency checks: company, order, chunking and B do not show.  The independent
reference is the pinned bits of the loops those entries ran before (tests/golden/logit_posterior_bits.npz), which
test_gpu_logit_posterior_bits.py holds every entry to.

One resident synthetic pair of 500 rows per width; idx1 is every third row (167 rows: a partial last row block of the fused
kernel, and rows shared with idx0)."""
import ctypes
import os
import sys

import numpy as np
import pytest

from flgp_amd import _lib, api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_logit_posterior as ref  # noqa: E402

pytestmark = pytest.mark.gpu

N = 500
TOL = 1e-5
IDX1 = np.arange(0, N, 3)                               # 167 rows, an index set
SIGMAS = [(0.0, 1e-3), (0.05, 0.0)]                     # sigma11, sigma22
TS5 = np.array([1.5, 4.0, 2.25, 3.0, 2.25])
COLS5 = np.array([0, 1, 2, 1, 2], dtype=np.int32)       # five problems over three columns; problems 2 and 4 are one problem


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()


def host_pair(n, width):
    rng = np.random.default_rng(1000 + width)
    values = np.sort(rng.uniform(0.4, 1.0, width))[::-1].copy()
    return values, np.asfortranarray(rng.standard_normal((n, width)))


@pytest.fixture(scope="module")
def pairs():
    """width -> (values, V, resident pair), made at first use and never written to"""
    made = {}

    def get(width, n=N):
        if (width, n) not in made:
            values, V = host_pair(n, width)
            made[(width, n)] = (values, V, api.ResidentEigenPair.from_host(api.EigenPair(values, V)))
        return made[(width, n)]
    yield get
    for _, _, rp in made.values():
        rp.free()


def rows0(m, kind, seed, n=N):
    rng = np.random.default_rng(seed)
    if kind == "range":
        start = int(rng.integers(0, n - m + 1))
        return np.arange(start, start + m)
    return rng.permutation(n)[:m]


def responses(m, seed, ncol=3):
    """m x ncol in [0, 1]: binary columns, the last one soft labels"""
    rng = np.random.default_rng(seed)
    Y = np.asfortranarray(rng.integers(0, 2, (m, ncol)).astype(np.float64))
    Y[:, ncol - 1] = rng.choice([0.0, 0.25, 0.75, 1.0], m)
    return Y


class Single:
    """The reference: the binary entry per (column, t), each made once and left unchanged."""

    def __init__(self, rp, K, idx0, idx1, Y, sig, max_iter=100):
        self.rp, self.K, self.idx0, self.idx1, self.Y = rp, K, idx0, idx1, Y
        self.s11, self.s22 = sig
        self.max_iter = max_iter
        self.done = {}

    def __call__(self, cols, ts):
        B = len(ts)
        mean = np.zeros((len(self.idx1), B), order="F"); cov = np.zeros((len(self.idx1), B), order="F")
        its = np.zeros(B, dtype=np.int32)
        for b, (c, t) in enumerate(zip(cols, ts)):
            key = (int(c), float(t))
            if key not in self.done:
                post, it = self.rp.logit_posterior(self.idx0, self.idx1, self.K, float(t), self.Y[:, int(c)], self.s11, self.s22,
                                                   tol=TOL, max_iter=self.max_iter, return_iters=True)
                self.done[key] = (post["mean"].copy(), post["cov"].copy(), it)
            mean[:, b], cov[:, b], its[b] = self.done[key]
        return mean, cov, its

    def batch(self, cols, ts, max_parallel=0):
        post, its = self.rp.logit_posterior_batch(self.idx0, self.idx1, self.K, ts, self.Y, col=cols, sigma11=self.s11,
                                                  sigma22=self.s22, tol=TOL, max_iter=self.max_iter, max_parallel=max_parallel,
                                                  return_iters=True)
        return post["mean"], post["cov"], its


def same_bits(got, want, what=""):
    (gm, gc, gi), (wm, wc, wi) = got, want
    assert gm.shape == wm.shape and gc.shape == wc.shape, what
    assert np.array_equal(gi, wi), (what, gi, wi)
    assert np.array_equal(gm, wm), (what, "mean", np.abs(gm - wm).max())
    assert np.array_equal(gc, wc), (what, "cov", np.abs(gc - wc).max())
    assert np.isfinite(gm).all() and np.isfinite(gc).all(), what


# ---- 1. each problem is the single entry ---------------------------------------------------------------------------------
# (40, 24), (40, 40): the dense route; (40, 41): the first weight-space shape; (15, 16), (16, 17), (17, 35): the operand's
# 16-row tile; (12, 257): a second 256-thread block and padded strides; (65, 66): a second Cholesky panel and a second
# block row of the triangular inverse; (129, 263): the fused kernel's 32-row block; (205, 206): its 16-row block
SHAPES = [(40, 24), (40, 40), (40, 41), (1, 2), (15, 16), (16, 17), (17, 35), (12, 257), (33, 300), (65, 66), (129, 263),
          (205, 206)]


@pytest.mark.parametrize("K,m", SHAPES)
def test_each_problem_is_the_single_entry(pairs, K, m):
    _, _, rp = pairs(K)
    for a, sig in enumerate(SIGMAS):
        kind = ("range", "perm")[(K + m + a) % 2]
        idx0 = rows0(m, kind, 31 * K + m + a)
        S = Single(rp, K, idx0, IDX1, responses(m, 7 * K + m), sig)
        same_bits(S.batch(COLS5, TS5), S(COLS5, TS5), f"K={K} m={m} {kind} sigma={sig}")


def test_new_rows_as_a_range(pairs):
    _, _, rp = pairs(33)
    idx1 = np.arange(N - 167, N)
    for K, m in ((33, 300), (33, 20)):
        S = Single(rp, K, rows0(m, "perm", 5), idx1, responses(m, 6), SIGMAS[0])
        same_bits(S.batch(COLS5, TS5), S(COLS5, TS5), f"m={m}")


# ---- 2. any B ------------------------------------------------------------------------------------------------------------
def test_any_batch_size(pairs):
    K, m = 16, 48
    _, _, rp = pairs(K)
    S = Single(rp, K, rows0(m, "perm", 11), IDX1, responses(m, 12), SIGMAS[1])
    rng = np.random.default_rng(13)
    grid = np.array([0.5, 1.5, 2.25, 3.0, 4.0, 8.0])
    for B in (1, 2, 7, 33):
        cols = rng.integers(0, 3, B).astype(np.int32); ts = grid[rng.integers(0, grid.size, B)]
        same_bits(S.batch(cols, ts), S(cols, ts), f"B={B}")
    # col None: one column per problem
    ts = np.array([1.5, 4.0, 2.25])
    post, its = rp.logit_posterior_batch(S.idx0, IDX1, K, ts, S.Y, sigma11=S.s11, sigma22=S.s22, tol=TOL, return_iters=True)
    same_bits((post["mean"], post["cov"], its), S(np.arange(3), ts), "col=None")


# ---- 3. company, order, chunks -------------------------------------------------------------------------------------------
def test_company_order_and_chunks_do_not_show(pairs):
    K, m = 65, 140
    _, _, rp = pairs(K)
    S = Single(rp, K, rows0(m, "range", 21), IDX1, responses(m, 22), SIGMAS[1])
    rng = np.random.default_rng(23)
    cols = np.array([0, 1, 2, 1, 2, 0, 2], dtype=np.int32); ts = np.array([1.5, 4.0, 2.25, 0.5, 2.25, 8.0, 3.0])
    want = S(cols, ts)
    first = S.batch(cols, ts, max_parallel=1)
    same_bits(first, want, "max_parallel=1")
    for mp in (2, 3, 0):
        got = S.batch(cols, ts, max_parallel=mp)
        assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes(), mp
        assert np.array_equal(got[2], first[2]), mp
    p = rng.permutation(7)
    gm, gc, gi = S.batch(cols[p], ts[p])
    same_bits((gm, gc, gi), (want[0][:, p], want[1][:, p], want[2][p]), "permuted")
    alone = S.batch(cols[3:4], ts[3:4])
    same_bits(alone, (want[0][:, 3:4], want[1][:, 3:4], want[2][3:4]), "alone")
    # duplicated problems give identical columns
    assert np.array_equal(first[0][:, 2], first[0][:, 4]) and np.array_equal(first[1][:, 2], first[1][:, 4])
    assert first[2][2] == first[2][4]


# ---- 4. problems leave the loop at different iterations --------------------------------------------------------------------
def no_step_near(steps, tol=TOL):
    """tests/test_gpu_logit_posterior.py: no step norm within a factor 3 of tol, so rounding cannot move the count"""
    return not any(tol / 3 <= s <= 3 * tol for s in steps)


MIXED = dict(K=16, m=48, rows_seed=41, y_seed=42, sig=(0.05, 1e-3), cols=np.array([0, 1, 2, 0, 1, 2], dtype=np.int32),
             ts=np.array([0.3, 0.3, 12.0, 200.0, 8.0, 100.0]))


def mixed_problem(values, V):
    """The problems of MIXED with the numpy loop's iteration counts and step norms."""
    c = MIXED
    idx0 = rows0(c["m"], "perm", c["rows_seed"]); Y = responses(c["m"], c["y_seed"])
    its, steps = [], []
    for col, t in zip(c["cols"], c["ts"]):
        _, _, it, st = ref.weight_space_mode(values, V, c["K"], t, idx0, Y[:, col], c["sig"][0], TOL)
        its.append(it); steps.append(st)
    return idx0, Y, np.array(its), steps


def test_problems_leave_the_loop_at_different_iterations(pairs):
    c = MIXED
    values, V, rp = pairs(c["K"])
    idx0, Y, its_np, steps = mixed_problem(values, V)
    assert all(no_step_near(s) for s in steps) and its_np.min() < its_np.max(), its_np
    S = Single(rp, c["K"], idx0, IDX1, Y, c["sig"])
    want = S(c["cols"], c["ts"])
    assert np.array_equal(want[2], its_np), (want[2], its_np)
    got = S.batch(c["cols"], c["ts"])
    same_bits(got, want)
    assert got[2].min() < got[2].max()
    # the cap stops some problems and not others (the two-iteration problem has converged when it is reached); reaching it
    # is not an error
    cap = 2
    assert its_np.min() == cap < its_np.max(), its_np
    S2 = Single(rp, c["K"], idx0, IDX1, Y, c["sig"], max_iter=cap)
    got2 = S2.batch(c["cols"], c["ts"])
    same_bits(got2, S2(c["cols"], c["ts"]), "max_iter=2")
    assert np.array_equal(got2[2], np.minimum(its_np, cap))


# ---- 5. one sequence of launches per iteration -----------------------------------------------------------------------------
def prof_count(name):
    c = ctypes.c_int(); ms = ctypes.c_double(); w = ctypes.c_double()
    _lib.lib().flgp_prof_query(name.encode(), ctypes.addressof(c), ctypes.addressof(ms), ctypes.addressof(w))
    return c.value


def test_an_iteration_is_one_sequence_for_the_whole_chunk(pairs):
    c = MIXED
    values, V, rp = pairs(c["K"])
    idx0, Y, _, _ = mixed_problem(values, V)
    S = Single(rp, c["K"], idx0, IDX1, Y, c["sig"])
    L = _lib.lib()
    L.flgp_prof_reset(); L.flgp_prof_enable(2)
    try:
        _, _, its = S.batch(c["cols"], c["ts"])
    finally:
        L.flgp_prof_enable(0)
    assert prof_count("logit_ws_batch_iter") == its.max() < its.sum()
    assert prof_count("logit_ws_newton_iter") == 0
    assert prof_count("gpc_predict_rows_multi") == 1
    L.flgp_prof_reset()


# ---- 6. the one-vs-rest entry ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,m", [(33, 300), (40, 24)])
def test_the_indicator_matrix_gives_the_multiclass_entry(pairs, K, m):
    _, _, rp = pairs(K)
    J = 5
    rng = np.random.default_rng(61 + m)
    labels = rng.integers(0, J, m).astype(np.float64)
    labels[labels == 3] = 4                                 # class 3 has no member
    assert not (labels == 3).any() and (labels == 4).any()
    idx0 = rows0(m, "perm", 62 + m)
    ts = 0.5 + 0.7 * np.arange(J)
    ind = np.asfortranarray((labels[:, None] == np.arange(J)[None, :]).astype(np.float64))
    for s11, s22 in SIGMAS:
        mc, its_mc = rp.logit_posterior_multiclass(idx0, IDX1, K, ts, labels, s22, sigma11=s11, tol=TOL, return_iters=True)
        post, its = rp.logit_posterior_batch(idx0, IDX1, K, ts, ind, sigma11=s11, sigma22=s22, tol=TOL, return_iters=True)
        assert post["mean"].tobytes() == mc["mean"].tobytes() and post["cov"].tobytes() == mc["cov"].tobytes()
        assert its.tobytes() == its_mc.astype(np.int32).tobytes()


# ---- 7. the wide route -----------------------------------------------------------------------------------------------------
def test_wide_route(pairs):
    K, m, n = 1030, 1031, 1100
    _, _, rp = pairs(K, n)
    idx1 = np.arange(0, n, 3)
    S = Single(rp, K, rows0(m, "perm", 71, n=n), idx1, responses(m, 72), SIGMAS[1])
    cols = np.array([0, 2], dtype=np.int32); ts = np.array([1.5, 4.0])
    same_bits(S.batch(cols, ts), S(cols, ts), "K=1030")


# ---- 8. not resting on one implementation ----------------------------------------------------------------------------------
def test_against_the_dense_restatement(pairs):
    K, m = 64, 133
    values, V, rp = pairs(K)
    s11, s22 = 1e-3, 1e-3
    idx0 = rows0(m, "perm", 85); Y = responses(m, 86)
    cols = np.array([0, 1, 2], dtype=np.int32); ts = np.array([1.5, 4.0, 2.25])
    post, its = rp.logit_posterior_batch(idx0, IDX1, K, ts, Y, col=cols, sigma11=s11, sigma22=s22, tol=TOL, return_iters=True)
    assert (post["cov"] >= s22).all()
    for b in range(3):
        mean, cov, C22, it, steps = ref.dense_posterior(values, V, K, ts[b], idx0, IDX1, Y[:, cols[b]], s11, s22, TOL)
        assert no_step_near(steps), steps
        atol_mean, atol_cov = ref.tolerances(mean, cov, C22, m)
        dm = np.abs(post["mean"][:, b] - mean).max(); dc = np.abs(post["cov"][:, b] - cov).max()
        print(f"problem {b}: |dmean| {dm:.3e} (atol {atol_mean:.3e})  |dcov| {dc:.3e} (atol {atol_cov:.3e})  iters {its[b]} / {it}")
        assert its[b] == it
        assert dm <= atol_mean and dc <= atol_cov, b


# ---- 9. a pivot that is not positive: the status and the naming, nothing else ------------------------------------------------
def test_a_bad_pivot_names_the_lowest_problem(pairs):
    """A pair with one value that is not a number: Q(0, 0) is not a number for every problem whose rows hold it, the first
    pivot test fails in the first iteration, and the entry reports the lowest problem with the binary entry's text."""
    K, m = 16, 48
    values, V = host_pair(N, K)
    V = V.copy(order="F"); V[7, 0] = np.nan
    rp = api.ResidentEigenPair.from_host(api.EigenPair(values, V))
    try:
        idx0 = np.arange(m); Y = responses(m, 91)
        with pytest.raises(api.FlgpError) as single:
            rp.logit_posterior(idx0, IDX1, K, 4.0, Y[:, 1], 0.0, 1e-3)
        assert single.value.code == -5
        for mp in (0, 1):
            with pytest.raises(api.FlgpError) as e:
                rp.logit_posterior_batch(idx0, IDX1, K, [4.0, 1.5, 2.25], Y, sigma22=1e-3, col=[1, 0, 2], max_parallel=mp)
            assert e.value.code == -5
            assert e.value.message == "problem 0 (t=4): " + single.value.message.replace("logit_posterior:", "logit_posterior_batch:")
            assert "Cholesky pivot 0 <= 0 in Newton iteration 1" in e.value.message
        # rows without the bad value: the handle still works
        idx0 = np.arange(100, 100 + m)
        post = rp.logit_posterior_batch(idx0, np.arange(200, 300), K, [4.0, 1.5], Y, col=[1, 0], sigma22=1e-3)
        assert np.isfinite(post["mean"]).all() and (post["cov"] >= 1e-3).all()
    finally:
        rp.free()
