"""Helpers and case tables of the logit-posterior bit tests (test_gpu_logit_posterior_bits.py, test_logit_posterior_case_table.py)
and of the recorder tests/golden/record_logit_posterior_bits.py.

* host_pair(), rows0(), responses(): the synthetic pairs, row sets and responses of test_gpu_logit_posterior_batch.py, with
  its seeds.
* CASES: the pinned cases.  A binary case is one (shape, row sets, sigma pair, max_iter) with its (column, t) problems; a
  class case is one one-vs-rest call; a failure case is a call that must be refused.  tests/golden/logit_posterior_bits.npz
  holds, per case, the bits of mean and cov (m_new x problems, column-major), the iteration counts and, for failures, the
  status and the text, as flgp_eigenpair_logit_posterior (binary cases) and flgp_eigenpair_logit_posterior_multiclass at
  max_parallel = 1 (class cases) returned them on an MI355X while each still ran a Newton loop of its own -- the
  implementations the batch entry was built to reproduce, recorded before they became the batch of one and of J.

The pinned cases read a short idx1 (every 13th row: 39 rows of the 500, an index set over one full 32-row block of the
fused kernel and a partial one) so that the fixture stays small; the long-idx1 row-block edges are covered by the
comparisons with the numpy restatement in the three test_gpu_logit_posterior*.py files.
"""
from __future__ import annotations

import os
from collections import namedtuple

import numpy as np

from flgp_amd import api

N = 500
TOL = 1e-5
SIGMAS = [(0.0, 1e-3), (0.05, 0.0)]                     # sigma11, sigma22
# (40, 24), (40, 40): the dense route; (40, 41), (1, 2): the first weight-space shapes; (15, 16), (16, 17), (17, 35): the
# operand's 16-row tile; (12, 257): a second 256-thread block and padded strides; (65, 66): a second Cholesky panel and a
# second block row of the triangular inverse; (129, 263), (205, 206): the fused kernel's 32- and 16-row blocks
SHAPES = [(40, 24), (40, 40), (40, 41), (1, 2), (15, 16), (16, 17), (17, 35), (12, 257), (33, 300), (65, 66), (129, 263),
          (205, 206)]
COLS4 = (0, 1, 2, 1)                                    # the distinct problems of the batch test's COLS5 / TS5
TS4 = (1.5, 4.0, 2.25, 3.0)
MIXED_COLS = (0, 1, 2, 0, 1, 2)                         # the batch test's MIXED: iteration counts from 2 up to the maximum
MIXED_TS = (0.3, 0.3, 12.0, 200.0, 8.0, 100.0)
WIDE = (1030, 1031, 1100)                               # K, m, n: the wide route
NAN_AT = (7, 0)                                         # the failure cases' pair holds one value that is not a number
BITS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "logit_posterior_bits.npz")
LARGEST_FIXTURE = 140707                                # bytes of the largest fixture before this one


def host_pair(n, width):
    rng = np.random.default_rng(1000 + width)
    values = np.sort(rng.uniform(0.4, 1.0, width))[::-1].copy()
    return values, np.asfortranarray(rng.standard_normal((n, width)))


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


def rows1(kind, n=N):
    """The short idx1: every 13th row, or the last 39 rows as a range."""
    return np.arange(0, n, 13) if kind == "set" else np.arange(n - 39, n)


# ------------------------------------------------------------------------------------------------- the pinned cases
# entry "binary": Y is responses(m, y_seed), the problems are (cols, ts).  entry "classes": the labels of class_labels(), J
# = len(ts) classes, cols is None.  fails: the pair has the value NAN_AT replaced and the call must be refused.
Case = namedtuple("Case", "key entry K m n kind0 rows_seed kind1 y_seed sig cols ts max_iter fails")


def _cases():
    out = []
    for K, m in SHAPES:
        for a, sig in enumerate(SIGMAS):
            kind = ("range", "perm")[(K + m + a) % 2]
            out.append(Case(f"binary-K{K}-m{m}-{kind}-s{a}", "binary", K, m, N, kind, 31 * K + m + a, "set", 7 * K + m, sig,
                            COLS4, TS4, 100, False))
    out.append(Case("binary-K33-m300-perm-s0-idx1range", "binary", 33, 300, N, "perm", 5, "range", 6, SIGMAS[0], COLS4, TS4,
                    100, False))
    for cap in (100, 2):
        out.append(Case(f"binary-mixed-K16-m48-maxiter{cap}", "binary", 16, 48, N, "perm", 41, "set", 42, (0.05, 1e-3),
                        MIXED_COLS, MIXED_TS, cap, False))
    K, m, n = WIDE
    out.append(Case(f"binary-wide-K{K}-m{m}", "binary", K, m, n, "perm", 71, "set", 72, SIGMAS[1], (0, 2), (1.5, 4.0), 100,
                    False))
    for K, m in ((33, 300), (40, 24)):                               # J = 5, class 3 without a member
        for a, sig in enumerate(SIGMAS):
            out.append(Case(f"classes-K{K}-m{m}-J5-s{a}", "classes", K, m, N, "perm", 62 + m, "set", 61 + m, sig, None,
                            tuple(0.5 + 0.7 * np.arange(5)), 100, False))
    out.append(Case("classes-K64-m450-J10", "classes", 64, 450, N, "perm", 3, "set", 4, (0.0, 1e-3), None,
                    tuple(0.5 + 0.7 * np.arange(10)), 100, False))
    out.append(Case("fails-binary-K16-m48", "binary", 16, 48, N, "first", 0, "set", 91, (0.0, 1e-3), (1,), (4.0,), 100, True))
    out.append(Case("fails-classes-K16-m48-J3", "classes", 16, 48, N, "first", 0, "set", 91, (0.0, 1e-3), None,
                    (4.0, 1.5, 2.25), 100, True))
    return out


CASES = _cases()


def class_labels(c):
    J = len(c.ts)
    rng = np.random.default_rng(c.y_seed)
    labels = rng.integers(0, J, c.m).astype(np.float64)
    if J == 5:
        labels[labels == 3] = 4                                   # class 3 has no member
    return labels


def case_inputs(c):
    """(idx0, idx1, Y) of a case: Y is the m x 3 response matrix of a binary case, the m labels of a class case."""
    idx0 = np.arange(c.m) if c.kind0 == "first" else rows0(c.m, c.kind0, c.rows_seed, n=c.n)
    return idx0, rows1(c.kind1, n=c.n), (responses(c.m, c.y_seed) if c.entry == "binary" else class_labels(c))


def indicator(labels, J):
    return np.asfortranarray((labels[:, None] == np.arange(J)[None, :]).astype(np.float64))


class Pairs:
    """(width, n, with the NaN or not) -> resident pair, made at first use and never written to"""

    def __init__(self):
        self.made = {}

    def __call__(self, c):
        key = (c.K, c.n, c.fails)
        if key not in self.made:
            values, V = host_pair(c.n, c.K)
            if c.fails:
                V = V.copy(order="F"); V[NAN_AT] = np.nan
            self.made[key] = api.ResidentEigenPair.from_host(api.EigenPair(values, V))
        return self.made[key]

    def free(self):
        for rp in self.made.values():
            rp.free()
        self.made = {}


def _guarded(c, call):
    """call() -> (mean, cov, iters, code, message); a refusal of a failure case gives empty arrays, its status and text."""
    try:
        mean, cov, its = call()
    except api.FlgpError as e:
        if not c.fails:
            raise
        return np.zeros((0, 0)), np.zeros((0, 0)), np.zeros(0, dtype=np.int32), e.code, e.message
    return np.asfortranarray(mean), np.asfortranarray(cov), np.asarray(its, dtype=np.int32), 0, ""


def run_binary(rp, c):
    """The binary entry over the problems of a binary case, one call per problem."""
    idx0, idx1, Y = case_inputs(c)

    def call():
        B = len(c.ts)
        mean = np.zeros((idx1.size, B), order="F"); cov = np.zeros((idx1.size, B), order="F"); its = np.zeros(B, dtype=np.int32)
        for b, (col, t) in enumerate(zip(c.cols, c.ts)):
            post, its[b] = rp.logit_posterior(idx0, idx1, c.K, float(t), Y[:, col], c.sig[0], c.sig[1], tol=TOL,
                                              max_iter=c.max_iter, return_iters=True)
            mean[:, b] = post["mean"]; cov[:, b] = post["cov"]
        return mean, cov, its
    return _guarded(c, call)


def run_batch(rp, c, max_parallel):
    """The batch entry on a case: its (cols, ts) problems, or the indicator matrix of a class case."""
    idx0, idx1, Y = case_inputs(c)
    cols = None if c.entry == "classes" else np.array(c.cols, dtype=np.int32)
    if c.entry == "classes":
        Y = indicator(Y, len(c.ts))

    def call():
        post, its = rp.logit_posterior_batch(idx0, idx1, c.K, np.array(c.ts), Y, col=cols, sigma11=c.sig[0], sigma22=c.sig[1],
                                             tol=TOL, max_iter=c.max_iter, max_parallel=max_parallel, return_iters=True)
        return post["mean"], post["cov"], its
    return _guarded(c, call)


def run_classes(rp, c, max_parallel):
    """The one-vs-rest entry on a class case."""
    idx0, idx1, labels = case_inputs(c)

    def call():
        post, its = rp.logit_posterior_multiclass(idx0, idx1, c.K, np.array(c.ts), labels, c.sig[1], sigma11=c.sig[0], tol=TOL,
                                                  max_iter=c.max_iter, max_parallel=max_parallel, return_iters=True)
        return post["mean"], post["cov"], its
    return _guarded(c, call)


Pinned = namedtuple("Pinned", "mean cov iters code message")


def load_bits():
    """{case key: Pinned(mean bits, cov bits (uint64, m_new x problems), iters (int32), code, message)} from the fixture,
    after checking that it is this table's."""
    with np.load(BITS_FILE) as z:
        keys = [str(k) for k in z["keys"]]
        assert keys == [c.key for c in CASES], "tests/golden/logit_posterior_bits.npz was recorded for another case table"
        out = {}
        for i, c in enumerate(CASES):
            B = 0 if c.fails else len(c.ts)
            rows = 0 if c.fails else rows1(c.kind1, n=c.n).size
            mean, cov, its = z[f"mean{i}"], z[f"cov{i}"], z[f"iters{i}"]
            assert mean.dtype == np.uint64 and cov.dtype == np.uint64 and mean.shape == cov.shape == (rows, B), c.key
            assert its.shape == (B,), c.key
            out[c.key] = Pinned(mean, cov, its.astype(np.int32), int(z["code"][i]), str(z["message"][i]))
    return out
