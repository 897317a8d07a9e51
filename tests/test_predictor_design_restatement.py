"""CPU: the numpy restatement of the greedy design (tests/np_predictor_design.py, the orders of DESIGN 8 f-25) computes what the
algebra says, on small random models (ELL rows on a random operand):

* the final scores against the dense conditional variance in long double (a Cholesky of Z_J Z_J^T + d I), and against
  |L^-1 z|^2 = z^T M^-1 z of f-24's M = I + Z_J^T Z_J / d (tests/np_predictor_update.py's solver), within the operation-count
  bound of f-25; the scores before every pick against the reference given the picks so far, within the bound at that t;
* every pick is optimal: its reference variance is at least the largest over the untaken rows minus twice the bound;
* the picks are distinct; gain is non-increasing -- exactly: a score only ever has a square subtracted, and the pick was the
  largest of the untaken scores, the next pick's among them;
* gain[t] is the score of picks[t] before step t, bit for bit; the twin of a duplicated row and all-zero rows behave as stated."""
import functools

import numpy as np
import pytest

import np_predictor_design as nd
import np_predictor_draws as npd
import np_predictor_update as npu
from flgp_amd import _lib

LD = nd.LD
MODELS = [(300, 5, 80, 20, 40, 0.1), (120, 3, 40, 8, 30, 0.05), (90, 10, 30, 30, 90, 1e-3)]


@functools.lru_cache(maxsize=None)
def model(n, r, s, K, B, d):
    rng = np.random.default_rng([n, r, s, K])
    idx = np.sort(np.stack([rng.permutation(s)[:r] for _ in range(n)]), axis=1).astype(np.int32)
    val = rng.uniform(0.0, 1.0, size=(n, r)); val /= val.sum(1, keepdims=True)
    P = rng.normal(size=(s, K + 3)) * 10.0 ** rng.uniform(-1.0, 0.3, size=(1, K + 3))
    picks, gain, score, before = nd.design(idx, val, P, K, d, B, trace=True)
    Z = npd.cols(idx, val, P, 0, K)
    absZ = npd.cols(idx, np.abs(val), np.abs(P), 0, K)
    for a in (idx, val, P, picks, gain, score, before, Z, absZ):
        a.setflags(write=False)
    return idx, val, P, picks, gain, score, before, Z, absZ


@pytest.mark.parametrize("n,r,s,K,B,d", MODELS)
def test_final_scores_against_both_dense_references(n, r, s, K, B, d):
    idx, val, P, picks, gain, score, before, Z, absZ = model(n, r, s, K, B, d)
    ref, alpha = nd.cond_var(Z, picks, d)
    bnd = nd.bound(absZ, picks, alpha, d, K, r)
    ratio = float((np.abs(score.astype(LD) - ref) / bnd).max())
    Zl = Z.astype(LD)
    M = np.eye(K, dtype=LD) + Zl[picks].T @ Zl[picks] / LD(d)
    via_m = (Zl.T * npu.ld_solve_spd(M, Zl.T)).sum(0)
    ratio_m = float((np.abs(score.astype(LD) - via_m) / bnd).max())
    print(f"n={n} K={K} B={B} d={d}: |score - ref| / bound = {ratio:.3e}, against z^T M^-1 z {ratio_m:.3e}, "
          f"references apart {float(np.abs(ref - via_m).max()):.1e}")
    assert ratio <= 1.0 and ratio_m <= 1.0
    assert float(np.abs(ref - via_m).max()) <= 1e-15 * float(np.abs(ref).max()) * (K + B)     # two routes to one long-double value


@pytest.mark.parametrize("n,r,s,K,B,d", MODELS)
def test_every_pick_is_optimal_and_the_running_scores_hold(n, r, s, K, B, d):
    idx, val, P, picks, gain, score, before, Z, absZ = model(n, r, s, K, B, d)
    worst = 0.0
    for t in range(B):
        ref, alpha = nd.cond_var(Z, picks[:t], d)
        bnd = nd.bound(absZ, picks[:t], alpha, d, K, r)
        worst = max(worst, float((np.abs(before[t].astype(LD) - ref) / bnd).max()))
        free = np.ones(n, dtype=bool); free[picks[:t]] = False
        j = picks[t]
        assert free[j]
        assert ref[j] >= (ref[free] - bnd[free]).max() - bnd[j], t            # within twice the bound of the largest
    print(f"n={n} K={K} B={B}: largest |running score - ref| / bound over the steps {worst:.3e}")
    assert worst <= 1.0


@pytest.mark.parametrize("n,r,s,K,B,d", MODELS)
def test_picks_are_distinct_and_gain_never_rises(n, r, s, K, B, d):
    idx, val, P, picks, gain, score, before, Z, absZ = model(n, r, s, K, B, d)
    assert len(set(picks.tolist())) == B and picks.min() >= 0 and picks.max() < n
    assert (np.diff(gain) <= 0).all()
    np.testing.assert_array_equal(gain, before[np.arange(B), picks])
    np.testing.assert_array_equal(before[0], nd.scores0(idx, val, P, K))
    assert (score <= before[0]).all()
    if B == n:
        assert sorted(picks.tolist()) == list(range(n))


def test_twins_and_zero_rows():
    n, r, s, K, B, d = 90, 10, 30, 30, 90, 1e-3
    idx, val, P = (np.array(a) for a in model(n, r, s, K, B, d)[:3])
    idx[57], val[57] = idx[11], val[11]                        # a twin
    val[[5, 40, 89]] = 0.0                                     # all-zero rows
    picks, gain, score, before = nd.design(idx, val, P, K, d, B, trace=True)
    order = {int(j): t for t, j in enumerate(picks)}
    assert order[11] < order[57]                               # equal scores take the lower index, and the twin stays eligible
    np.testing.assert_array_equal(before[:, 11][:order[11] + 1], before[:, 57][:order[11] + 1])
    assert picks[-3:].tolist() == [5, 40, 89] and (gain[-3:] == 0.0).all() and (gain[:-3] > 0.0).all()
    assert (before[:, [5, 40, 89]] == 0.0).all() and (score[[5, 40, 89]] == 0.0).all()


def test_the_library_has_the_loop_this_restates():
    assert hasattr(_lib.lib(), "flgp_dev_predictor_design_rows") and "flgp_dev_predictor_design_rows" in _lib.declared_symbols()


def test_the_argmax_order():
    nan = float("nan")
    s = np.array([1.0, 3.0, nan, 3.0, -np.inf])
    none = np.zeros(5, dtype=bool)
    assert nd.argbest(s, none) == 1
    assert nd.argbest(s, np.array([0, 1, 0, 0, 0], dtype=bool)) == 3
    assert nd.argbest(s, np.array([1, 1, 0, 1, 0], dtype=bool)) == 4          # a NaN is never larger, not even than -inf
    assert nd.argbest(s, np.array([1, 1, 0, 1, 1], dtype=bool)) == 2          # and is taken when nothing else is left
    np.testing.assert_array_equal(nd.lane_sum(np.arange(130.0)[None, :]), [130 * 129 / 2])
