"""Helpers and case table of the Polya-Gamma bit tests (test_gpu_pg_bits.py, test_pg_predict_case_table.py) and of the
recorder tests/golden/record_pg_predict_bits.py.

* host_pair(), rows(), responses(), class_labels(): the synthetic pair of test_gpu_pg_batch.py (500 rows, its seeds), the
  row sets and the label columns.
* CASES: the pinned cases.  A binary case is one (K, m, sigma_nv) with three (column, t, seed) chains; a class case is one
  one-vs-rest call.  tests/golden/pg_predict_bits.npz holds, per binary case, the bits of pi_pred, Y_pred (m_new x 3), omega
  and f (m x 3) and, per class case, the bits of probs (m_new x J) and labels, as flgp_eigenpair_pg_predict and
  flgp_eigenpair_pg_predict_multiclass returned them on an MI355X while they still ran a Woodbury sweep of their own, one
  chain after another -- the implementation the batch entry was built to reproduce, recorded before the two became the
  batch of one and of J.

The new rows are a short idx1 (every 13th row: 39 of the 500) so that the fixture stays small, and idx0 always holds three
of them, so that sigma_nv's match term has entries.
"""
from __future__ import annotations

import os
from collections import namedtuple

import numpy as np

from flgp_amd import api

N = 500
N_SAMPLE = 6
SIGMA = 2e-2
SIGMA_NVS = (0.0, 1e-2)
# (40, 24), (40, 40): the m x m route; (40, 41): the first Woodbury shape; (16, 48); (12, 257): a second 256-thread block,
# m no multiple of 32 (padded slot strides); (33, 300): K no multiple of 32; (65, 66): one column past the Cholesky panel
SHAPES = [(40, 24), (40, 40), (40, 41), (16, 48), (12, 257), (33, 300), (65, 66)]
TS3 = (1.5, 4.0, 2.25)                                  # the three chains of a binary case: columns 0, 1 (binary), 2 (soft)
SEEDS3 = (11, 2 ** 63 + 5, 2 ** 64 - 1)
BITS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pg_predict_bits.npz")
BINARY_KEYS = ("pi_pred", "Y_pred", "omega", "f")

Case = namedtuple("Case", "key entry K m sigma_nv ts seed")     # seed: the three seeds of a binary case, the one of a class case


def _cases():
    out = []
    for K, m in SHAPES:
        for a, snv in enumerate(SIGMA_NVS):
            out.append(Case(f"binary-K{K}-m{m}-nv{a}", "binary", K, m, snv, TS3, SEEDS3))
    for K, m in ((24, 20), (12, 60)):
        out.append(Case(f"classes-K{K}-m{m}-J3", "classes", K, m, 0.0, (1.5, 2.5, 4.0), 500))
    # class 3 has no member; seed + j wraps past 2^64 at j = 2
    out.append(Case("classes-K40-m41-J4-wrap", "classes", 40, 41, 0.0, (1.5, 2.5, 4.0, 3.0), 2 ** 64 - 2))
    return out


CASES = _cases()


def pair_width(K):
    return 40 if K <= 40 else K


def host_pair(width):
    """synthetic_pair(500, width, seed=1600 + width, scale=0.5) of test_gpu_pg_batch.py"""
    rng = np.random.default_rng(1600 + width)
    values = np.sort(rng.uniform(0.4, 1.0, width))[::-1].copy()
    return values, np.asfortranarray(0.5 * rng.standard_normal((N, width)))


def rows(c):
    """(idx0, idx1): idx1 is every 13th row; idx0 is three rows of idx1 and m - 3 of the others, shuffled."""
    idx1 = np.arange(0, N, 13, dtype=np.int32)
    rng = np.random.default_rng(1000 * c.K + c.m)
    idx0 = np.concatenate([rng.choice(idx1, 3, replace=False),
                           rng.choice(np.setdiff1d(np.arange(N), idx1), c.m - 3, replace=False)])
    return rng.permutation(idx0).astype(np.int32), idx1


def responses(c):
    """m x 3 in [0, 1]: two binary columns and one of soft labels"""
    rng = np.random.default_rng(7 * c.K + c.m)
    Y = np.asfortranarray((rng.uniform(size=(c.m, 3)) < 0.45).astype(np.float64))
    Y[:, 2] = rng.choice([0.0, 0.25, 0.75, 1.0], c.m)
    return Y


def class_labels(c):
    """m labels in 0 .. 2, whatever J is: with J = 4 class 3 has no member"""
    return np.random.default_rng(32 + c.m).integers(0, 3, c.m).astype(np.float64)


class Pairs:
    """width -> resident pair, made at first use and never written to"""

    def __init__(self):
        self.made = {}

    def __call__(self, c):
        w = pair_width(c.K)
        if w not in self.made:
            self.made[w] = api.ResidentEigenPair.from_host(api.EigenPair(*host_pair(w)))
        return self.made[w]

    def free(self):
        for rp in self.made.values():
            rp.free()
        self.made = {}


def run_binary(rp, c):
    """The binary entry, one call per chain of a binary case -> {key: m_new x 3 or m x 3}"""
    idx0, idx1 = rows(c)
    Y = responses(c)
    out = {"pi_pred": np.zeros((idx1.size, 3), order="F"), "Y_pred": np.zeros((idx1.size, 3), order="F"),
           "omega": np.zeros((c.m, 3), order="F"), "f": np.zeros((c.m, 3), order="F")}
    for b in range(3):
        one = rp.test_pgbinary(idx0, idx1, c.K, c.ts[b], Y[:, b], SIGMA, c.sigma_nv, N_sample=N_SAMPLE, output_pi=True,
                               seed=c.seed[b], return_state=True)
        for k in BINARY_KEYS:
            out[k][:, b] = one[k]
    return out


def run_batch(rp, c, max_parallel):
    """The batch entry on a binary case: its three chains as one call"""
    idx0, idx1 = rows(c)
    return rp.test_pgbinary_batch(idx0, idx1, c.K, c.ts, responses(c), SIGMA, c.sigma_nv, seeds=list(c.seed),
                                  N_sample=N_SAMPLE, max_parallel=max_parallel, output_pi=True, return_state=True)


def run_classes(rp, c):
    """The one-vs-rest entry on a class case -> {"probs": m_new x J, "labels": m_new}"""
    idx0, idx1 = rows(c)
    labels, probs = rp.predict_logit_mult_gp_cpp(idx0, idx1, c.K, np.array(c.ts), class_labels(c), SIGMA, N_sample=N_SAMPLE,
                                                 seed=c.seed, output_probs=True)
    return {"probs": probs, "labels": labels}


def run_classes_batch(rp, c, max_parallel):
    """The batch entry's one-vs-rest wrapper on a class case"""
    idx0, idx1 = rows(c)
    labels, probs = rp.predict_logit_mult_gp_batch(idx0, idx1, c.K, np.array(c.ts), class_labels(c), SIGMA, N_sample=N_SAMPLE,
                                                   seed=c.seed, output_probs=True, max_parallel=max_parallel)
    return {"probs": probs, "labels": labels}


def out_keys(c):
    return BINARY_KEYS if c.entry == "binary" else ("probs", "labels")


def out_shape(c, k):
    mnew = len(range(0, N, 13))
    if c.entry == "binary":
        return (c.m if k in ("omega", "f") else mnew, 3)
    return (mnew, len(c.ts)) if k == "probs" else (mnew,)


def bits(a):
    return np.asfortranarray(a).view(np.uint64)


def load_bits():
    """{case key: {output: uint64 bit patterns}} from the fixture, after checking that it is this table's."""
    with np.load(BITS_FILE) as z:
        assert [str(k) for k in z["keys"]] == [c.key for c in CASES], \
            "tests/golden/pg_predict_bits.npz was recorded for another case table"
        out = {}
        for i, c in enumerate(CASES):
            out[c.key] = {k: z[f"{k}{i}"] for k in out_keys(c)}
            for k, a in out[c.key].items():
                assert a.dtype == np.uint64 and a.shape == out_shape(c, k), (c.key, k)
    return out
