"""GPU (-m gpu): flgp_dev_predictor_rows (csrc/predictor.hip) alone, on random ELL rows and a random P in padded, canaried
buffers.  Per shape: mean and var bit for bit against the numpy restatement of the stated order (tests/np_predictor.py);
independently of that order |var - exact| <= (K + 2 r + 4) 2^-53 (cg + sum_k (sum_a |A P|)^2), exact and the bound in
np.longdouble -- the standard forward bound of r-term chains followed by a sum of K non-negative squares; var >= cg exactly;
canaries and padding untouched; rows 0 .. 63 of an n = 257 call equal the n = 64 call bit for bit; d_mean = NULL and
d_var = NULL each leave the other output's bits unchanged.

The kernel has one dispatch path: a wave per (row, group) walks ceil((K + q) / 64) column chunks.  K + q = 1+0, 1+1: one
partial chunk; 62+1, 63+1: the mean in the last lanes of a full chunk; 64+1: the mean alone in a second chunk; 127+2: the
mean straddles a chunk edge; 200+17: four chunks, a partial last one.  n = 1, 63, 64, 65, 257 cross the four rows of a
workgroup and more than one workgroup; r = 1, 3, 10, 32 = FLGP_RMAX; s = 40; groups 1 and 3."""
import numpy as np
import pytest
import torch

import np_predictor as npp
from flgp_amd import _lib
from predictor_cases import GROUPS, KQ, NS, RS, S          # tests/test_predictor_case_table.py: what these shapes reach

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NMAX = max(NS)


def _inputs(K, q, groups, r):
    rng = np.random.default_rng([K, q, groups, r])
    idx = np.sort(np.stack([rng.permutation(S)[:r] for _ in range(NMAX)]), axis=1).astype(np.int32)
    val = rng.normal(size=(NMAX, r)) * 10.0 ** rng.uniform(-2.0, 2.0, size=(NMAX, r))     # mixed signs and magnitudes
    w = groups * (K + q)
    ldp = w + 5
    P = np.full((S, ldp), np.nan)
    P[:, :w] = rng.normal(size=(S, w))
    cg = rng.uniform(1e-3, 1.0, groups)
    return idx, val, P, ldp, cg


def _run(idx, val, P, ldp, cg, n, groups, K, q, want_mean=True, want_var=True):
    """one call on the first n rows; the outputs sit in NaN with leading dimensions n + 3 / n + 2 and a spare column"""
    L = _lib.lib()
    r = idx.shape[1]
    d_idx = torch.from_numpy(idx[:n].copy()).to(DEV); d_val = torch.from_numpy(val[:n].copy()).to(DEV)
    d_P = torch.from_numpy(P).to(DEV); d_cg = torch.from_numpy(cg).to(DEV)
    ldm, ldv = n + 3, n + 2
    d_mean = torch.full((groups * q + 1, ldm), float("nan"), dtype=torch.float64, device=DEV)
    d_var = torch.full((groups + 1, ldv), float("nan"), dtype=torch.float64, device=DEV)
    rc = L.flgp_dev_predictor_rows(None, d_idx.data_ptr(), d_val.data_ptr(), n, r, d_P.data_ptr(), ldp, S, groups, K, q,
                                   d_cg.data_ptr(), d_mean.data_ptr() if want_mean else None, ldm,
                                   d_var.data_ptr() if want_var else None, ldv)
    assert rc == 0, L.flgp_last_error().decode()
    torch.cuda.synchronize()
    mean, var = d_mean.cpu().numpy(), d_var.cpu().numpy()
    # canaries: the spare column and the rows past n of every column; the inputs as they were
    assert np.isnan(mean[:, n:]).all() and np.isnan(mean[groups * q:]).all()
    assert np.isnan(var[:, n:]).all() and np.isnan(var[groups:]).all()
    if not want_mean:
        assert np.isnan(mean).all()
    if not want_var:
        assert np.isnan(var).all()
    np.testing.assert_array_equal(d_P.cpu().numpy(), P)
    np.testing.assert_array_equal(d_idx.cpu().numpy(), idx[:n]); np.testing.assert_array_equal(d_val.cpu().numpy(), val[:n])
    return mean[:groups * q, :n].T, var[:groups, :n].T


def _forward_bound(idx, val, P, cg, groups, K, q):
    """exact var and the bound, in np.longdouble"""
    ld = np.longdouble
    n, r = idx.shape
    w = K + q
    exact = np.zeros((n, groups), dtype=ld); bound = np.zeros((n, groups), dtype=ld)
    for g in range(groups):
        terms = val.astype(ld)[:, :, None] * P[idx, g * w:g * w + K].astype(ld)         # n x r x K
        exact[:, g] = ld(cg[g]) + (terms.sum(1) ** 2).sum(1)
        bound[:, g] = ld(K + 2 * r + 4) * ld(2.0) ** -53 * (ld(cg[g]) + (np.abs(terms).sum(1) ** 2).sum(1))
    return exact, bound


@pytest.mark.parametrize("groups", GROUPS)
@pytest.mark.parametrize("K,q", KQ, ids=["K%d+q%d" % kq for kq in KQ])
def test_rows_match_the_stated_order_bit_for_bit(K, q, groups):
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    for r in RS:
        idx, val, P, ldp, cg = _inputs(K, q, groups, r)
        ref_mean, ref_var = npp.rows(idx, val, P, groups, K, q, cg)
        exact, bound = _forward_bound(idx, val, P, cg, groups, K, q)
        got = {}
        for n in NS:
            mean, var = got[n] = _run(idx, val, P, ldp, cg, n, groups, K, q, want_mean=q > 0)
            np.testing.assert_array_equal(var, ref_var[:n], err_msg=f"var r={r} n={n}")                       # 2
            if q:
                np.testing.assert_array_equal(mean, ref_mean[:n], err_msg=f"mean r={r} n={n}")               # 1
            err = np.abs(var.astype(np.longdouble) - exact[:n])
            assert (err <= bound[:n]).all(), (r, n, float((err / bound[:n]).max()))                         # 3
            assert (var >= cg[None, :]).all()                                                                 # 4
        np.testing.assert_array_equal(got[257][1][:64], got[64][1])                                           # 6
        np.testing.assert_array_equal(got[257][0][:64], got[64][0])
        if q:                                                                                                 # 7
            n = 65
            mean_only, _ = _run(idx, val, P, ldp, cg, n, groups, K, q, want_var=False)
            _, var_only = _run(idx, val, P, ldp, cg, n, groups, K, q, want_mean=False)
            np.testing.assert_array_equal(mean_only, got[n][0])
            np.testing.assert_array_equal(var_only, got[n][1])


def test_the_restated_order_is_not_the_only_one_the_bound_admits():
    """the bit test above would pass vacuously if every order gave the same bits: at K = 200, r = 10 a plain k-ascending sum
    of the squares differs from the stated lane order in some row"""
    idx, val, P, ldp, cg = _inputs(200, 17, 1, 10)
    _, var = npp.rows(idx, val, P, 1, 200, 17, cg)
    z = np.zeros((NMAX, 200))
    for a in range(10):
        z = z + val[:, a:a + 1] * P[idx[:, a], :200]
    plain = np.zeros(NMAX)
    for k in range(200):
        plain = plain + z[:, k] * z[:, k]
    assert (cg[0] + plain != var[:, 0]).any()
