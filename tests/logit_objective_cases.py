"""Helpers and case tables of the logit-objective tests (test_gpu_logit_objective_batch.py, test_gpu_logit_objective_bits.py)
and of the recorder tests/golden/record_logit_objective_bits.py.

* synthetic_pair(), rows(), responses(): the resident pair, the row sets and the responses the GPU tests run on.
* GROUPS: the pinned cases.  A group is one (shape, row kind, sigma, configuration, max_iter); its problems are every
  column of its Y at every t of TS (problems()).  tests/golden/logit_objective_bits.npz holds, per problem, the bits of the
  value and the iteration count that flgp_eigenpair_logit_objective returned on an MI355X while it still ran a Newton loop
  of its own (GpcLowRank for m > K, hk_c11 + logit_la_on_device for m <= K) -- the implementation the batch entry was built
  to reproduce, recorded before the single entry became the batch of one.
"""
from __future__ import annotations

import os
from collections import namedtuple

import numpy as np

from flgp_amd import api

N_ROWS, N_COLS = 3000, 240
PAIR_SEED = 21
TS = (0.3, 1.0, 4.0, 20.0)
PRIOR = (0.5, 3.0, 1.5)
LOWRANK_SHAPES = [(64, 65), (65, 300), (200, 201), (200, 1000)]     # (K, m): one row above K, K off the 64-column panel,
#                                                                     one and four Cholesky panels
DENSE_SHAPES = [(50, 40), (200, 200), (65, 1)]                       # m <= K: the dense loop
BITS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "logit_objective_bits.npz")


def synthetic_pair(n, K, seed):
    rng = np.random.default_rng(seed)
    values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
    V = np.asfortranarray(rng.standard_normal((n, K)))
    return api.EigenPair(values, V), api.ResidentEigenPair.from_host(api.EigenPair(values, V))


def rows(n, m, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "perm":
        return rng.permutation(n)[:m]
    idx = rng.integers(0, n, m)                                  # repeated rows
    idx[m // 2:] = idx[: m - m // 2]
    return idx


def responses(m, seed, singleton=True):
    """Y (m x 6): the one-vs-rest indicators of five classes (class 4 with a single member when the rows allow it), then a
    binomial column for N in 1..5 -- under that N the indicator columns are valid responses too."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, 4 if singleton and m >= 5 else 5, m)
    if singleton and m >= 5:
        labels[rng.integers(0, m)] = 4
    N = rng.integers(1, 6, m).astype(np.float64)
    Y = np.zeros((m, 6), order="F")
    Y[:, :5] = labels[:, None] == np.arange(5)[None, :]
    Y[:, 5] = rng.binomial(N.astype(int), 0.35)
    return labels, Y, N


# ------------------------------------------------------------------------------------------------- the pinned cases
# config "indicator": the five indicator columns, N = NULL, approach "marginal"; "binomial": all six columns under the
# binomial N, approach "posterior" with PRIOR -- the two configurations of the batch tests.
Group = namedtuple("Group", "key K m kind sigma config max_iter row_seed resp_seed singleton")


def _groups():
    out = []
    for K, m in LOWRANK_SHAPES:
        for kind in ("perm", "repeated"):
            for sigma in (1e-3, 0.1):
                for config in ("indicator", "binomial"):
                    out.append(Group(f"lowrank-K{K}-m{m}-{kind}-s{sigma:g}-{config}", K, m, kind, sigma, config, 100,
                                     31 * K + m, 7 * K + m, True))
    for K, m in DENSE_SHAPES:                                      # the batch test's sigma per configuration
        for sigma, config in ((1e-3, "indicator"), (0.1, "binomial")):
            out.append(Group(f"dense-K{K}-m{m}-perm-s{sigma:g}-{config}", K, m, "perm", sigma, config, 100,
                             61 * K + m, 62 * K + m, True))
    for K, m in LOWRANK_SHAPES:                                    # every problem stops at the cap
        out.append(Group(f"lowrank-K{K}-m{m}-perm-s0.001-indicator-maxiter2", K, m, "perm", 1e-3, "indicator", 2,
                         41 * K + m, 43 * K + m, False))
    return out


GROUPS = _groups()


def group_inputs(g):
    """(idx, Y, N, keyword arguments) of a group, as ResidentEigenPair.logit_objective[_batch] takes them."""
    idx = rows(N_ROWS, g.m, g.kind, g.row_seed)
    _, Y, N = responses(g.m, g.resp_seed, singleton=g.singleton)
    if g.config == "indicator":
        return idx, Y[:, :5], None, dict(sigma=g.sigma, approach="marginal", prior=None, max_iter=g.max_iter)
    return idx, Y, N, dict(sigma=g.sigma, approach="posterior", prior=PRIOR, max_iter=g.max_iter)


def problems(g):
    """(cols, ts) of a group: every column at every t of TS, column by column."""
    ncol = 5 if g.config == "indicator" else 6
    return np.repeat(np.arange(ncol, dtype=np.int32), len(TS)), np.tile(np.array(TS), ncol)


def run_single(rp, g):
    """The single entry over the problems of a group: (values, iters)."""
    idx, Y, N, kw = group_inputs(g)
    cols, ts = problems(g)
    out = [rp.logit_objective(float(t), g.K, idx, Y[:, int(c)], N=N, return_iters=True, **kw) for c, t in zip(cols, ts)]
    return np.array([v for v, _ in out], dtype=np.float64), np.array([i for _, i in out], dtype=np.int32)


def load_bits():
    """{group key: (value bits as uint64, iters as int32)} from the fixture, after checking that it is this table's."""
    with np.load(BITS_FILE) as z:
        keys = [str(k) for k in z["keys"]]
        assert keys == [g.key for g in GROUPS], "tests/golden/logit_objective_bits.npz was recorded for another case table"
        out = {}
        for i, g in enumerate(GROUPS):
            sel = z["group"] == i
            cols, ts = problems(g)
            assert np.array_equal(z["col"][sel], cols) and np.array_equal(z["t"][sel], ts), g.key
            out[g.key] = (z["bits"][sel].astype(np.uint64), z["iters"][sel].astype(np.int32))
    return out
