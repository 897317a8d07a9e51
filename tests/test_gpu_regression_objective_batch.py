"""GPU: the regression training objective for B (pair, x) problems in one call (flgp_regression_batch_*).
The contract is bit for bit: every value and gradient of a batch is what the single entry
(flgp_eigenpair_regression_objective) returns for that pair at that x, whatever shares the call.  The single entry is now
the batch of one, so these tests compare a problem in company with the same problem alone; the independent reference is
the pinned fixture tests/golden/regression_objective_bits.npz, which test_gpu_regression_objective_bits.py holds both
entries to on this file's shapes.  No tolerance appears in the bit tests; one test ties the batch to the numpy
restatement."""
import os
import sys

import numpy as np
import pytest

from flgp_amd import _lib, api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_regression_objective as R  # noqa: E402

pytestmark = pytest.mark.gpu

N, KP = 3000, 200
SIGMA = 1e-5


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()


@pytest.fixture(scope="module")
def pairs():
    """Three different pairs of the same size: (values, V, resident pair) each."""
    made = []
    for seed in (21, 22, 23):
        values, V = R.synthetic_pair(N, KP, np.random.default_rng(seed))
        made.append((values, V, api.ResidentEigenPair.from_host(api.EigenPair(values, V))))
    yield made
    for _, _, rp in made:
        rp.free()


def rows(kind, m, rng):
    return np.arange(100, 100 + m) if kind == "range" else rng.choice(N, m, replace=False)


def draw_x(noise, m, rng):
    t = rng.uniform(0.5, 4.0)
    return np.r_[t, rng.uniform(0.05, 0.5)] if noise == "same" else np.r_[t, rng.uniform(0.05, 0.4, m)]


def single(rp, x, K, idx, Y, noise, approach, grad, sigma=SIGMA):
    """The reference: one call of the single entry.  (value, grad or None)"""
    if grad:
        return rp.regression_objective(x, K, idx, Y, sigma=sigma, noise=noise, approach=approach)
    return rp.regression_objective(x, K, idx, Y, sigma=sigma, noise=noise, approach=approach, grad=False), None


def same_bits(got, want):
    """got: (value, grad row or None) of one position of a batch; want: single()'s result"""
    assert got[0] == want[0], (got[0], want[0])
    if want[1] is not None:
        assert np.array_equal(got[1], want[1]), np.abs(got[1] - want[1]).max()


def run_batch(ctx, X, prob=None, grad=True):
    if grad:
        v, g = ctx(X, prob=prob)
        return [(v[a], g[a]) for a in range(v.size)]
    v = ctx(X, prob=prob, grad=False)
    return [(v[a], None) for a in range(v.size)]


class Problems:
    """B problems on the cycled pairs (so one pair carries several x), their x and the single entry's results."""

    def __init__(self, pairs, B, K, m, q, noise, approach, grad, seed, kind="scattered", max_parallel=0):
        rng = np.random.default_rng(seed)
        self.K, self.noise, self.approach, self.grad = K, noise, approach, grad
        self.idx = rows(kind, m, rng)
        self.Y = rng.standard_normal((m, q))
        self.rps = [pairs[b % len(pairs)][2] for b in range(B)]
        self.host = [pairs[b % len(pairs)][:2] for b in range(B)]
        self.X = np.array([draw_x(noise, m, rng) for _ in range(B)])
        self.ctx = api.RegressionObjectiveBatch(self.rps, K, self.idx, self.Y, sigma=SIGMA, noise=noise, approach=approach,
                                                max_parallel=max_parallel)
        self._ref = {}

    def ref(self, b, x=None, grad=None):
        x = self.X[b] if x is None else x
        grad = self.grad if grad is None else grad
        key = (b, x.tobytes(), grad)
        if key not in self._ref:
            self._ref[key] = single(self.rps[b], x, self.K, self.idx, self.Y, self.noise, self.approach, grad)
        return self._ref[key]

    def prefix(self, B):
        """a context of its own on the first B problems"""
        return api.RegressionObjectiveBatch(self.rps[:B], self.K, self.idx, self.Y, sigma=SIGMA, noise=self.noise,
                                            approach=self.approach)

    def check_all(self):
        got = run_batch(self.ctx, self.X, grad=self.grad)
        for b in range(len(self.rps)):
            same_bits(got[b], self.ref(b))
        return got


# one row above K, K on and off the 64-wide panel, one to four panels and triangular-inverse block rows, m across a change
# of the split-K plan
WOODBURY = [(1, 2), (64, 65), (65, 300), (129, 130), (200, 201), (200, 1000), (63, 2500)]


@pytest.mark.parametrize("noise", ["same", "different"])
@pytest.mark.parametrize("K,m", WOODBURY, ids=[f"K{k}-m{m}" for k, m in WOODBURY])
def test_bit_for_bit_against_the_single_entry(pairs, K, m, noise):
    """q in {1, 3, 70} (70 crosses the 64-wide tile of the K x q products), both approaches, with and without the gradient,
    B in {1, 2, 7, 33}: the 33 problems of a (q, approach) are drawn once and a context of B takes the first B."""
    case = WOODBURY.index((K, m))
    for qi, q in enumerate((1, 3, 70)):
        for ai, approach in enumerate(("marginal", "posterior")):
            kind = "range" if (case + qi + ai) % 3 == 0 else "scattered"
            P = Problems(pairs, 33, K, m, q, noise, approach, True, seed=1000 * case + 10 * q + ai, kind=kind)
            try:
                for B in (1, 2, 7, 33):
                    ctx = P.ctx if B == 33 else P.prefix(B)
                    try:
                        assert (ctx.B, ctx.nx, ctx.chunk) == (B, m + 1 if noise == "different" else 2, B)
                        for grad in (True, False):
                            for b, got in enumerate(run_batch(ctx, P.X[:B], grad=grad)):
                                same_bits(got, P.ref(b, grad=grad))
                    finally:
                        if ctx is not P.ctx:
                            ctx.free()
            finally:
                P.ctx.free()


@pytest.mark.parametrize("noise", ["same", "different"])
def test_chunks_do_not_change_the_bits(pairs, noise):
    """B = 7 with max_parallel = 3: chunks of 3, 3 and 1"""
    P = Problems(pairs, 7, 65, 300, 3, noise, "posterior", True, seed=77, max_parallel=3)
    whole = api.RegressionObjectiveBatch(P.rps, 65, P.idx, P.Y, sigma=SIGMA, noise=noise, approach="posterior")
    try:
        assert P.ctx.chunk == 3 and whole.chunk == 7
        got = P.check_all()
        for a, w in zip(got, run_batch(whole, P.X)):
            same_bits(a, w)
    finally:
        P.ctx.free(); whole.free()


@pytest.mark.parametrize("noise", ["same", "different"])
def test_company_and_order_do_not_change_the_bits(pairs, noise):
    P = Problems(pairs, 7, 129, 300, 3, noise, "posterior", True, seed=5, max_parallel=4)
    try:
        first = P.check_all()
        for a, w in zip(P.check_all(), first):                   # a second eval on the same handle
            same_bits(a, w)
        perm = np.array([4, 0, 6, 2, 5, 1, 3])
        for a, b in zip(run_batch(P.ctx, P.X[perm], prob=perm), perm):
            same_bits(a, P.ref(b))
        sub = np.array([5, 2])                                    # a strict subset
        for a, b in zip(run_batch(P.ctx, P.X[sub], prob=sub), sub):
            same_bits(a, P.ref(b))
        rep = np.array([3, 3, 1, 3, 0, 1, 6, 6, 2])              # repeats (A > B), some at another x
        Xr = P.X[rep].copy()
        rng = np.random.default_rng(9)
        for a in (1, 5, 7):
            Xr[a] = draw_x(noise, 300, rng)
        for a, (got, b) in enumerate(zip(run_batch(P.ctx, Xr, prob=rep), rep)):
            same_bits(got, P.ref(b, Xr[a]))
        v = P.ctx(P.X[sub], prob=sub, grad=False)                 # values only, after gradients on the same buffers
        assert [v[0], v[1]] == [P.ref(5)[0], P.ref(2)[0]]
    finally:
        P.ctx.free()


@pytest.mark.parametrize("max_parallel", [1, 3])
@pytest.mark.parametrize("noise", ["same", "different"])
@pytest.mark.parametrize("K,m", [(50, 40), (200, 200), (65, 1)], ids=["K50-m40", "K200-m200", "K65-m1"])
def test_direct_route(pairs, K, m, noise, max_parallel):
    """m <= K: the problems are dealt to the pool's workers; the single entry is one such item on one worker"""
    for kind, approach, grad in (("scattered", "posterior", True), ("range", "marginal", True), ("scattered", "marginal", False)):
        P = Problems(pairs, 7, K, m, 3, noise, approach, grad, seed=K + m, kind=kind, max_parallel=max_parallel)
        try:
            assert P.ctx.chunk == max_parallel
            P.check_all()
            sub = np.array([6, 1, 1])
            for a, b in zip(run_batch(P.ctx, P.X[sub], prob=sub, grad=grad), sub):
                same_bits(a, P.ref(b))
        finally:
            P.ctx.free()


@pytest.fixture(scope="module")
def singular_pair():
    """values[0] = values[1] = 1 and columns 0 and 1 the same +-1 vector on the 256 rows used below: with x = (t, 0) and
    sigma = 1e-300, l = 1 exactly, M00 = M10 = M11 = 256 exactly and the second pivot is 256 + 1e-300 - 16^2 = 0 in fp64."""
    rng = np.random.default_rng(31)
    values, V = R.synthetic_pair(N, 65, rng)
    idx = rng.choice(N, 256, replace=False)
    values = values.copy(); values[:2] = 1.0
    V = V.copy(order="F")
    V[idx, 0] = V[idx, 1] = np.where(rng.random(256) < 0.5, -1.0, 1.0)
    rp = api.ResidentEigenPair.from_host(api.EigenPair(values, V))
    yield rp, idx
    rp.free()


def test_one_failing_problem_leaves_the_others_alone(pairs, singular_pair):
    bad, idx = singular_pair
    K, sigma = 65, 1e-300
    rng = np.random.default_rng(32)
    Y = rng.standard_normal((256, 2))
    rps = [pairs[0][2], pairs[1][2], bad, pairs[2][2], pairs[0][2]]
    X = np.array([[2.0, 0.2], [1.5, 0.3], [2.0, 0.0], [3.0, 0.1], [0.7, 0.25]])
    with pytest.raises(api.FlgpError) as e:      # the precondition: the single entry refuses the problem
        bad.regression_objective(X[2], K, idx, Y, sigma=sigma, noise="same", approach="marginal")
    assert e.value.code == -5
    ctx = api.RegressionObjectiveBatch(rps, K, idx, Y, sigma=sigma, noise="same", approach="marginal")
    try:
        v, g, status = ctx(X, return_status=True)
        assert status.tolist() == [0, 0, -5, 0, 0]
        assert np.isnan(v[2]) and np.isnan(g[2]).all()
        for a in (0, 1, 3, 4):
            same_bits((v[a], g[a]), single(rps[a], X[a], K, idx, Y, "same", "marginal", True, sigma=sigma))
        v, status = ctx(X, grad=False, return_status=True)
        assert status.tolist() == [0, 0, -5, 0, 0] and np.isnan(v[2])
        with pytest.raises(api.FlgpError) as e:  # status = NULL: the lowest failing position is reported
            ctx(X)
        assert e.value.code == -5 and e.value.message.startswith("position 2: regression_objective_batch:")
        assert "not positive definite" in e.value.message
    finally:
        ctx.free()


def close(dev, ref):
    """test_gpu_regression_objective.py's bounds: 1e-9 relative on the value, 1e-8 on the gradient"""
    (v, g), (vr, gr) = dev, ref
    assert abs(v - vr) <= 1e-9 * abs(vr), (v, vr)
    assert np.abs(g - gr).max() <= 1e-8 * max(1.0, np.abs(gr).max()), np.abs(g - gr).max()


@pytest.mark.parametrize("noise", ["same", "different"])
def test_against_the_restatement(pairs, noise):
    """The batch is tied to the reference's formulas and not only to its sibling."""
    P = Problems(pairs, 7, 65, 300, 3, noise, "posterior", True, seed=61)
    try:
        got = run_batch(P.ctx, P.X)
        for b in range(7):
            values, V = P.host[b]
            close(got[b], R.objective(values, V, 65, P.idx, P.Y, P.X[b], SIGMA, noise, "posterior"))
    finally:
        P.ctx.free()


def test_convenience_on_one_pair(pairs):
    _, _, rp = pairs[1]
    rng = np.random.default_rng(71)
    idx = rows("scattered", 150, rng)
    Y = rng.standard_normal((150, 2))
    xs = np.array([draw_x("same", 150, rng) for _ in range(4)])
    v, g = rp.regression_objective_batch(xs, 48, idx, Y)
    for a in range(4):
        same_bits((v[a], g[a]), rp.regression_objective(xs[a], 48, idx, Y))


def test_refusals(pairs):
    rps = [p[2] for p in pairs]
    rng = np.random.default_rng(81)
    values, V = R.synthetic_pair(100, 10, rng)
    small = api.ResidentEigenPair.from_host(api.EigenPair(values, V))
    idx = np.arange(10)
    Y = np.zeros(10)
    who = "regression_objective_batch"
    try:
        with pytest.raises(api.FlgpError) as e:
            api.RegressionObjectiveBatch(rps, KP + 1, idx, Y)
        assert e.value.code == -1 and e.value.message == f"problem 0: {who}: bad shape (K={KP + 1} of {KP}, m=10, q=1)"
        with pytest.raises(api.FlgpError) as e:                  # a pair whose K is too small for the shared K
            api.RegressionObjectiveBatch([rps[0], small, rps[1]], 11, idx, Y)
        assert e.value.code == -1 and e.value.message == f"problem 1: {who}: bad shape (K=11 of 10, m=10, q=1)"
        with pytest.raises(api.FlgpError) as e:                  # a pair whose n is too small for the shared idx
            api.RegressionObjectiveBatch([rps[0], rps[1], small], 4, np.r_[idx[:-1], 100], Y)
        assert e.value.code == -1 and e.value.message == f"problem 2: {who}: idx[9]=100 out of range"
        with pytest.raises(api.FlgpError) as e:
            api.RegressionObjectiveBatch(rps, 4, np.r_[idx[:-1], N], Y)
        assert e.value.code == -1 and "out of range" in e.value.message
        with pytest.raises(api.FlgpError) as e:
            api.RegressionObjectiveBatch(rps, 4, idx, Y, noise="equal")
        assert e.value.code == -3 and e.value.message == "The noise setting is illegal!"
        with pytest.raises(api.FlgpError) as e:
            api.RegressionObjectiveBatch(rps, 4, idx, Y, approach="bayes")
        assert e.value.code == -3 and e.value.message == "This model selection approach is not supported!"
        with pytest.raises(ValueError):
            api.RegressionObjectiveBatch(rps, 4, idx, np.zeros(9))
        # the library's own refusals of an evaluation, through the raw entry (the wrapper refuses the same things first)
        ctx = api.RegressionObjectiveBatch(rps, 4, idx, Y)
        try:
            L = _lib.lib()
            X = np.array([[2.0, 0.2], [2.0, 0.2], [2.0, 0.2]])
            v = np.zeros(3); g = np.zeros((3, 2)); prob = np.array([0, 3, 1], dtype=np.int32)

            def raw(A, Xa, prob=None, ldx=2, values=v):
                return L.flgp_regression_batch_eval(ctx._h, None if prob is None else prob.ctypes.data, A, Xa.ctypes.data, ldx,
                                                    None if values is None else values.ctypes.data, g.ctypes.data, 2, None)

            assert raw(3, X) == 0
            assert raw(0, X) == -1 and L.flgp_last_error().decode() == f"{who}: A=0 problems"
            assert raw(2, X) == -1 and L.flgp_last_error().decode() == f"{who}: prob may be NULL only if A == B (A=2, B=3)"
            assert raw(3, X, values=None) == -1 and "null pointer" in L.flgp_last_error().decode()
            assert raw(3, X, ldx=1) == -1
            assert L.flgp_last_error().decode() == f'{who}: noise "same" takes 2 parameters, not 1'
            assert raw(3, X, prob=prob) == -1
            assert L.flgp_last_error().decode() == f"position 1: {who}: prob=3 is outside [0, B=3)"
            for x, text in (([2.0, np.nan], "x must be finite"), ([2.0, -1.0], "x[1] + sigma must be positive"),
                            ([0.0, 0.2], 't = x[0] must be positive under "posterior"')):
                Xb = X.copy(); Xb[2] = x
                assert raw(3, Xb) == -1 and L.flgp_last_error().decode() == f"position 2: {who}: {text}"
                with pytest.raises(api.FlgpError) as e:
                    ctx(Xb)
                assert e.value.code == -1 and e.value.message == f"position 2: {who}: {text}"
            with pytest.raises(api.FlgpError) as e:
                ctx(np.ones((3, 3)))                                   # nx = 3 for "same"
            assert e.value.code == -1
        finally:
            ctx.free()
    finally:
        small.free()
