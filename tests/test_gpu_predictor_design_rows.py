"""GPU (-m gpu): flgp_dev_predictor_design_rows (csrc/predictor_design.hip) alone, on random ELL rows in padded,
canaried buffers: P is NaN from column K on (ldp = K + q + 5), picks, gain and score have canary tails, the workspace a NaN tail.
Shapes: tests/predictor_design_cases.py (what they reach: tests/test_predictor_design_case_table.py).

* picks, gain and score are bit for bit the restatement's (tests/np_predictor_design.py: the documented orders), on every shape,
  with the knob predictor_design_grid at 0 and again capped so that a workgroup walks several ranges and fewer partials exist;
* a second call gives the same bits; inputs and canaries are untouched; so do the rows read in place (knob
  predictor_design_pack = 0) instead of from their transposed copy;
* a pool with a duplicated row: equal scores take the lower index and the twin stays eligible; all-zero rows have score 0 and are
  never picked before a positive one; B = n exhausts the pool and every row appears once."""
import functools

import numpy as np
import pytest
import torch

import np_predictor_design as nd
import predictor_design_cases as dc
from flgp_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _problem(n, r, s, K, special=False):
    """(idx, val, P): mixed signs and magnitudes; `special`: a duplicated row and all-zero rows"""
    rng = np.random.default_rng([n, r, s, K, int(special)])
    if r <= s:
        idx = np.sort(np.stack([rng.permutation(s)[:r] for _ in range(n)]), axis=1).astype(np.int32)
    else:
        idx = np.sort(rng.integers(0, s, size=(n, r)), axis=1).astype(np.int32)
    val = rng.normal(size=(n, r)) * 10.0 ** rng.uniform(-1.0, 0.5, size=(n, r)) / r
    if special:
        idx[n - 7], val[n - 7] = idx[3], val[3]
        val[[2, n // 2, n - 1]] = 0.0
    W = K + dc.Q
    P = np.full((s, W + dc.LDP_PAD), np.nan)
    P[:, :K] = rng.normal(size=(s, K)) * 10.0 ** rng.uniform(-1.0, 0.5, size=(1, K))
    for a in (idx, val, P):
        a.setflags(write=False)
    return idx, val, P


@functools.lru_cache(maxsize=None)
def _want(n, r, s, K, B, special=False):
    idx, val, P = _problem(n, r, s, K, special)
    out = nd.design(idx, val, P, K, dc.D, B)
    for a in out:
        a.setflags(write=False)
    return out


class _Dev:
    def __init__(self, idx, val, P):
        up = lambda a: torch.from_numpy(np.array(a)).to(DEV)
        self.idx, self.val, self.P = up(idx), up(val), up(P)
        self.host = (idx, val, P)

    def untouched(self):
        for d, h in zip((self.idx, self.val, self.P), self.host):
            np.testing.assert_array_equal(d.cpu().numpy(), h)


def _run(D, n, r, s, K, B, knob=0, outputs=True):
    L = _lib.lib()
    need = L.flgp_dev_predictor_design_workspace(n, r, s, K, B)
    assert need == dc.workspace_bytes(n, r, s, K, B)
    picks = torch.full((B + 3,), -7, dtype=torch.int32, device=DEV)
    gain = torch.full((B + 3,), float("nan"), dtype=torch.float64, device=DEV)
    score = torch.full((n + 3,), float("nan"), dtype=torch.float64, device=DEV)
    work = torch.full((need // 8 + 64,), float("nan"), dtype=torch.float64, device=DEV)
    L.flgp_set_tuning(b"predictor_design_grid", knob)
    try:
        rc = L.flgp_dev_predictor_design_rows(None, D.idx.data_ptr(), D.val.data_ptr(), n, r, D.P.data_ptr(), K + dc.Q + dc.LDP_PAD, s, K, dc.D,
                                              B, picks.data_ptr(), gain.data_ptr() if outputs else None,
                                              score.data_ptr() if outputs else None, work.data_ptr(), need)
        assert rc == 0, L.flgp_last_error().decode()
        torch.cuda.synchronize()
    finally:
        L.flgp_set_tuning(b"predictor_design_grid", 0)
    assert (picks[B:] == -7).all().item() and torch.isnan(gain[B:]).all().item() and torch.isnan(score[n:]).all().item()
    assert torch.isnan(work[need // 8:]).all().item()
    if not outputs:
        assert torch.isnan(gain).all().item() and torch.isnan(score).all().item()
    return picks[:B].cpu().numpy(), gain[:B].cpu().numpy(), score[:n].cpu().numpy()


def _same(got, want, label):
    for g, w, name in zip(got, want, ("picks", "gain", "score")):
        np.testing.assert_array_equal(g, w, err_msg=f"{label}: {name}")


@pytest.mark.parametrize("n,r,s,K,B", dc.CASES)
def test_bit_for_bit_under_both_grid_settings(n, r, s, K, B):
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    D = _Dev(*_problem(n, r, s, K))
    want = _want(n, r, s, K, B)
    assert len(set(want[0].tolist())) == B
    _same(_run(D, n, r, s, K, B), want, "knob 0")
    for knob in dc.caps(n):
        _same(_run(D, n, r, s, K, B, knob), want, f"knob {knob}")
    _same(_run(D, n, r, s, K, B), want, "a second call")
    D.untouched()


@pytest.mark.parametrize("n,r,s,K,B", [(65, 32, 200, 65, 65), (1000, 10, 200, 64, 67), (257, 3, 20481, 4, 7)])
def test_rows_read_in_place_give_the_same_bits(n, r, s, K, B):
    """knob predictor_design_pack = 0: no transposed copy, the row-major arrays are read as they are"""
    D = _Dev(*_problem(n, r, s, K))
    L = _lib.lib()
    L.flgp_set_tuning(b"predictor_design_pack", 0)
    try:
        for knob in [0] + dc.caps(n):
            _same(_run(D, n, r, s, K, B, knob), _want(n, r, s, K, B), f"in place, knob {knob}")
    finally:
        L.flgp_set_tuning(b"predictor_design_pack", 1)
    D.untouched()


def test_gain_and_score_may_be_null():
    n, r, s, K, B = 257, 10, 200, 15, 257
    D = _Dev(*_problem(n, r, s, K))
    np.testing.assert_array_equal(_run(D, n, r, s, K, B, outputs=False)[0], _want(n, r, s, K, B)[0])


@pytest.mark.parametrize("n,r,s,K", [(257, 10, 200, 15), (1000, 3, 200, 65)])
def test_twins_zero_rows_and_an_exhausted_pool(n, r, s, K):
    idx, val, P = _problem(n, r, s, K, True)
    D = _Dev(idx, val, P)
    want = _want(n, r, s, K, n, True)
    picks, gain, score = _run(D, n, r, s, K, n, knob=2)
    _same((picks, gain, score), want, "special rows")
    assert sorted(picks.tolist()) == list(range(n))                                # exhausted: every row once
    order = {int(j): t for t, j in enumerate(picks)}
    assert order[3] < order[n - 7]                                                 # the lower index first; the twin is picked later
    zeros = sorted([2, n // 2, n - 1])
    assert picks[-3:].tolist() == zeros and (gain[-3:] == 0.0).all() and (gain[:-3] > 0.0).all() and (score[zeros] == 0.0).all()
    assert (np.diff(gain) <= 0).all()
    D.untouched()
