"""Helpers and case table of test_gpu_regression_objective_bits.py, test_regression_objective_case_table.py and of the
recorder tests/golden/record_regression_objective_bits.py.

* synthetic_pairs(): the three n = 3000, K = 200 pairs of test_gpu_regression_objective_batch.py.
* CASES: the pinned calls.  A case is one (pair, x) on one (route, K, m, noise, approach, q, row kind); the two or one draws
  of a configuration share idx and Y and differ in the pair and the x, so a context of the three pairs holds them all.
  FAILURES: the two calls pinned as outcomes.
* tests/golden/regression_objective_bits.npz holds, per case, the bits of the value (called with the gradient and value
  only) and of the gradient that flgp_eigenpair_regression_objective returned on an MI355X while it still ran Woodbury
  steps of its own (RgEval::woodbury_terms) -- the implementation the batch entry was built to reproduce, recorded before
  the single entry became the batch of one.
"""
from __future__ import annotations

import os
from collections import namedtuple

import numpy as np

import np_regression_objective as R
from flgp_amd import api

N, KP = 3000, 200
PAIR_SEEDS = (21, 22, 23)
SIGMA = 1e-5
# (K, m), m > K: one row above K, K on and off the 64-wide panel, one to four panels, m across a change of the split-K plan
WOODBURY = [(1, 2), (64, 65), (65, 300), (129, 130), (200, 201), (200, 1000), (63, 2500)]
DIRECT = [(50, 40), (200, 200), (65, 1)]                            # m <= K
QS = (1, 3, 70)                                                     # 70 crosses the 64-wide tile of the K x q products
KINDS = ("range", "scattered")
BITS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regression_objective_bits.npz")

Case = namedtuple("Case", "key route K m noise approach q kind pair seed x_seed")
Failure = namedtuple("Failure", "key K m")


def _cases():
    out = []
    for route, shapes in (("woodbury", WOODBURY), ("direct", DIRECT)):
        for noise in ("same", "different"):
            j = 0                                                  # q and the row kind rotate within a (route, noise)
            for K, m in shapes:
                for approach in ("marginal", "posterior"):
                    q, kind = QS[j % 3], KINDS[j % 2]
                    draws = 1 if (noise == "different" and m == 2500) else 2     # bounds the fixture's size
                    for d in range(draws):
                        out.append(Case(f"{route}-K{K}-m{m}-{noise}-{approach}-q{q}-{kind}-p{(j + d) % 3}", route, K, m, noise,
                                        approach, q, kind, (j + d) % 3, 1000 * K + m + 7 * j, 100 * (1000 * K + m) + 10 * j + d))
                    j += 1
    return out


CASES = _cases()
FAILURES = [Failure("failure-singular-pair-K65-m256", 65, 256), Failure("failure-five-rows-K48-m5", 48, 5)]


def synthetic_pairs():
    """[(values, V, resident pair)] for the seeds 21, 22, 23; the caller frees the resident pairs."""
    made = []
    for seed in PAIR_SEEDS:
        values, V = R.synthetic_pair(N, KP, np.random.default_rng(seed))
        made.append((values, V, api.ResidentEigenPair.from_host(api.EigenPair(values, V))))
    return made


def inputs(case):
    """(idx, Y, x) of a case; idx and Y depend on the configuration only, x on the draw."""
    rng = np.random.default_rng(case.seed)
    idx = np.arange(100, 100 + case.m) if case.kind == "range" else rng.choice(N, case.m, replace=False)
    Y = rng.standard_normal((case.m, case.q))
    rng = np.random.default_rng(case.x_seed)
    t = rng.uniform(0.5, 4.0)
    x = np.r_[t, rng.uniform(0.05, 0.5)] if case.noise == "same" else np.r_[t, rng.uniform(0.05, 0.4, case.m)]
    return idx, Y, x


def run_single(pairs, case):
    """The single entry: (value, value of the value-only call, gradient)."""
    idx, Y, x = inputs(case)
    rp = pairs[case.pair][2]
    kw = dict(sigma=SIGMA, noise=case.noise, approach=case.approach)
    v, g = rp.regression_objective(x, case.K, idx, Y, **kw)
    return v, rp.regression_objective(x, case.K, idx, Y, grad=False, **kw), g


def run_batch(pairs, case, B=1):
    """The same call through a context: of the case's pair alone (B = 1), or of the three pairs, evaluated at the case's
    pair only (B = 3)."""
    idx, Y, x = inputs(case)
    rps = [pairs[case.pair][2]] if B == 1 else [p[2] for p in pairs]
    prob = np.array([0 if B == 1 else case.pair], dtype=np.int32)
    ctx = api.RegressionObjectiveBatch(rps, case.K, idx, Y, sigma=SIGMA, noise=case.noise, approach=case.approach)
    try:
        v, g = ctx(x[None, :], prob=prob)
        return v[0], ctx(x[None, :], prob=prob, grad=False)[0], g[0]
    finally:
        ctx.free()


def failure_problem(f):
    """(values, V, K, idx, Y, x, sigma) of a failure case, both "same" and "marginal".

    failure-singular-pair: values[0] = values[1] = 1 and columns 0 and 1 the same +-1 vector on the 256 rows: with
    x = (2, 0) and sigma = 1e-300 the second pivot of the system matrix is 0 in fp64 (singular_pair of
    test_gpu_regression_objective_batch.py).  failure-five-rows: a repeated row with noise + sigma = 1e-300 on the direct
    route (test_singular_system_is_reported_or_finite of test_gpu_regression_objective.py)."""
    x = np.array([2.0, 0.0])
    if f.key == "failure-singular-pair-K65-m256":
        rng = np.random.default_rng(31)
        values, V = R.synthetic_pair(N, 65, rng)
        idx = rng.choice(N, 256, replace=False)
        values = values.copy(); values[:2] = 1.0
        V = V.copy(order="F")
        V[idx, 0] = V[idx, 1] = np.where(rng.random(256) < 0.5, -1.0, 1.0)
        return values, V, 65, idx, np.random.default_rng(32).standard_normal((256, 2)), x, 1e-300
    values, V = R.synthetic_pair(N, 48, np.random.default_rng(5))
    return values, V, 48, np.array([5, 9, 5, 17, 40]), np.arange(5.0), x, 1e-300


def run_failure(f, batch=False):
    """(code, message, value, value-only value, gradient): code 0 with numbers, or the error's code and text with NaNs."""
    values, V, K, idx, Y, x, sigma = failure_problem(f)
    rp = api.ResidentEigenPair.from_host(api.EigenPair(values, V))
    ctx = None
    try:
        if batch:
            ctx = api.RegressionObjectiveBatch([rp], K, idx, Y, sigma=sigma, noise="same", approach="marginal")
            v, g = ctx(x[None, :])
            return 0, "", v[0], ctx(x[None, :], grad=False)[0], g[0]
        v, g = rp.regression_objective(x, K, idx, Y, sigma=sigma, noise="same", approach="marginal")
        return 0, "", v, rp.regression_objective(x, K, idx, Y, sigma=sigma, noise="same", approach="marginal", grad=False), g
    except api.FlgpError as e:
        return e.code, e.message, np.nan, np.nan, np.zeros(0)
    finally:
        if ctx is not None:
            ctx.free()
        rp.free()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1)).view(np.uint64)


def load_bits():
    """{key: (value bits, value-only bits, gradient bits, code, message)} from the fixture, after checking that it is this
    table's."""
    with np.load(BITS_FILE) as z:
        keys = [str(k) for k in z["keys"]]
        assert keys == [c.key for c in CASES + FAILURES], \
            "tests/golden/regression_objective_bits.npz was recorded for another case table"
        off = z["grad_offsets"]
        return {k: (z["value_bits"][i], z["value_only_bits"][i], z["grad_bits"][off[i]:off[i + 1]], int(z["code"][i]),
                    str(z["message"][i])) for i, k in enumerate(keys)}
