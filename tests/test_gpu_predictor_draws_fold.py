"""GPU (-m gpu): the two kernels of flgp_predictor_draws_create (csrc/predictor_cols.hip) through
flgp_dev_predictor_draws_fold, on a random source operand P in padded buffers (NaN behind the groups' columns of P, NaN behind
the ncol columns of P_draw, which must stay).  Shapes: tests/predictor_draws_cases.py.

* P_draw is bit for bit the restatement's fold (tests/np_predictor_draws.py) fed the device's own normals;
* columns do not depend on S: draw t of S = 1, 5, 64 is draw t of S = 65, in P_draw and in the normals;
* the normals against flgp_amd/synth.py: |xi_dev - xi_numpy| <= 24 * 2^-53 * sqrt(-2 log u1) per entry.  The uniforms are exact on
  both sides (integer arithmetic and one exact scaling).  With u = 2^-53 and both libraries' log and cos within 1 ulp (their
  documented bounds, not measured here -- the assumption f-22 makes for exp): rad = sqrt(-2 log u1) carries 1 ulp of the log,
  halved by the root, and the root's own rounding, on each side: 2 (0.5 + 0.5) u = 2u relative between the two; the argument
  2 pi u2 is rounded once on each side (the two products may differ by 1 ulp of an argument below 2 pi: 2^-50 absolute, which
  |sin| <= 1 turns into at most 8u of the cosine), each cos adds 1 ulp (2u between the two) and each product 0.5u (1u): in
  units of rad, 2u + 8u + 2u + 1u = 13u <= 24u.  The largest observed ratio is printed (recorded in DESIGN f-23)."""
import functools

import numpy as np
import pytest
import torch

import np_predictor_draws as npd
import predictor_draws_cases as pc
from flgp_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x9E3779B97F4A7C15                                    # above 2^63: the seed is unsigned
U24 = 24.0 * 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _source(s, K, groups, q):
    rng = np.random.default_rng([s, K, groups, q])
    w = groups * (K + q)
    P = np.full((s, w + 3), np.nan)
    P[:, :w] = rng.normal(size=(s, w)) * 10.0 ** rng.uniform(-1.0, 1.0, size=(s, w))
    P.setflags(write=False)
    return P


def _fold(P, groups, K, q, S, seed=SEED):
    """(P_draw s x ncol, xi K x ncol) of one call; P_draw sits in NaN at ldd = ncol + 5 with a spare row"""
    L = _lib.lib()
    s, ldp = P.shape
    ncol = groups * q * S
    ldd = ncol + 5
    d_P = torch.from_numpy(np.array(P)).to(DEV)
    d_xi = torch.full((K + 1, ncol), float("nan"), dtype=torch.float64, device=DEV)
    d_Pd = torch.full((s + 1, ldd), float("nan"), dtype=torch.float64, device=DEV)
    rc = L.flgp_dev_predictor_draws_fold(None, d_P.data_ptr(), ldp, s, groups, K, q, S, seed, d_xi.data_ptr(), d_Pd.data_ptr(), ldd)
    assert rc == 0, L.flgp_last_error().decode()
    torch.cuda.synchronize()
    Pd, xi = d_Pd.cpu().numpy(), d_xi.cpu().numpy()
    assert np.isnan(Pd[:, ncol:]).all() and np.isnan(Pd[s]).all() and np.isnan(xi[K]).all()       # canaries
    assert not np.isnan(Pd[:s, :ncol]).any() and not np.isnan(xi[:K]).any()
    np.testing.assert_array_equal(d_P.cpu().numpy(), P)
    return Pd[:s, :ncol], xi[:K]


def _check(s, K, groups, q, draws):
    P = _source(s, K, groups, q)
    got, worst = {}, 0.0
    for S in draws:
        Pd, xi = got[S] = _fold(P, groups, K, q, S)
        label = f"s={s} K={K} groups={groups} q={q} S={S}"
        np.testing.assert_array_equal(Pd, npd.fold(P, groups, K, q, S, xi), err_msg=label)
        ref, rad = npd.normals(SEED, K, groups, q, S), npd.radius(SEED, K, groups, q, S)
        ratio = (np.abs(xi - ref) / (U24 * rad)).max()
        assert ratio <= 1.0, (label, ratio)
        worst = max(worst, ratio)
    big = max(draws)
    for S in draws:
        for gc in range(groups * q):
            for arr in (0, 1):
                np.testing.assert_array_equal(got[S][arr][:, gc * S:(gc + 1) * S], got[big][arr][:, gc * big:gc * big + S],
                                              err_msg=f"S={S} against S={big}, output {gc}")
    return worst


@pytest.mark.parametrize("K", pc.FOLD_K)
def test_fold_matches_the_restatement_and_columns_do_not_depend_on_S(K):
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    worst = 0.0
    for s in pc.FOLD_S:
        for groups, q in pc.FOLD_GQ:
            worst = max(worst, _check(s, K, groups, q, pc.FOLD_DRAWS))
    print(f"K={K}: largest |xi_dev - xi_numpy| / (24 * 2^-53 * sqrt(-2 log u1)) = {worst:.3f}")


def test_more_than_one_workgroup_of_columns():
    for s, K, (groups, q), S in pc.FOLD_EXTRA:
        worst = _check(s, K, groups, q, [5, S])
        print(f"s={s} K={K} q={q} S={S}: largest normal ratio {worst:.3f}")


def test_another_seed_gives_other_draws():
    P = _source(7, 5, 1, 3)
    a, xa = _fold(P, 1, 5, 3, 5)
    b, xb = _fold(P, 1, 5, 3, 5, seed=SEED + 1)
    assert (xa != xb).all() and (a != b).all()
    again, xc = _fold(P, 1, 5, 3, 5)
    np.testing.assert_array_equal(again, a); np.testing.assert_array_equal(xc, xa)
