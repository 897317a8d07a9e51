"""GPU (-m gpu): flgp_dev_nystrom_predictor_rows (csrc/nystrom_predictor.hip) alone, on a random Gaussian cloud, anchors, w, P
and cg in padded, canaried buffers (ldx, ldm, ldv > n).  The shapes are those of tests/nystrom_predictor_cases.py
(tests/test_nystrom_predictor_case_table.py: what they reach); every shape runs with both outputs, the mean alone and the
variance alone.

Reference: the np.longdouble restatement (tests/np_nystrom_predictor.py).  Forward bound, computed from the inputs (DESIGN 8
f-21 has the derivation), with u = 2^-53:
    S_ij   = |x_i|^2 + 2 sum_k |x_ik u_jk| + |u_j|^2
    eta_i  = max_j (dpad + 4) u S_ij inv_c + 3 u            the relative error of a similarity value
    M_ic   = f_i sum_j Z_ij |P_jc|
    |d mean_ic| <= b_ic = (3 eta_i + (3 s + 12) u) M_ic
    |d var_i|   <= sum_k (2 M_ik b_ik + b_ik^2) + (K + 8) u sum_k M_ik^2 + u cg
The test is not empty: max|mean| > 0, bound <= 1e-9 max|mean|, every row's sum_j Z_ij > 1e-200, no case skipped.
Bit checks, needing no reference: 513 rows as one call, in blocks of 256, one row at a time, with nystrom_dot_gemm 0 and 1
(d <= 64) and with T held one group at a time give identical bits; each output's bits do not depend on the other being
asked for; var >= cg; canaries and inputs untouched."""
import functools

import numpy as np
import pytest
import torch

import np_nystrom_predictor as nnp
import nystrom_predictor_cases as nc
from flgp_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A2 = 0.7
LD = np.longdouble
EPS = LD(2.0) ** -53


@functools.lru_cache(maxsize=None)
def inputs(n, d, s, K, q, groups):
    """the cloud, the anchors (rows of another draw of the cloud plus noise), inv_c = 1 / (a2 mean D_UU), w, P, cg; read-only"""
    rng = np.random.default_rng([n, d, s, K, q, groups])
    X = rng.normal(size=(n, d))
    U = rng.normal(size=(s, d)) if s > n else X[rng.permutation(n)[:s]] + 0.01 * rng.normal(size=(s, d))
    uu = (U * U).sum(1)
    mean_d = ((-2.0 * U @ U.T + uu[:, None]) + uu[None, :]).sum() / (s * s)
    inv_c = 1.0 / (A2 * mean_d) if mean_d > 0 else 1.0 / (A2 * 2.0 * d)          # (s = 1: the one anchor is at distance 0 of itself)
    Zuu = np.exp(-((-2.0 * U @ U.T + uu[:, None]) + uu[None, :]) * inv_c)
    w = 1.0 / (Zuu.sum(1) + 1e-9)
    wd = groups * (K + q)
    ldp = wd + 5
    P = np.full((s, ldp), np.nan)
    P[:, :wd] = rng.normal(size=(s, wd))
    cg = rng.uniform(1e-3, 1.0, groups)
    for a in (X, U, w, P, cg):
        a.setflags(write=False)
    return X, U, inv_c, w, P, ldp, cg


def run(X, U, inv_c, w, P, ldp, cg, groups, K, q, want_mean=True, want_var=True):
    """one call on all rows of X; the outputs sit in NaN with leading dimensions n + 3 / n + 2 and a spare column"""
    L = _lib.lib()
    n, d = X.shape
    s = U.shape[0]
    ldx, ldu, ldm, ldv = n + 1, s + 2, n + 3, n + 2
    dX = torch.full((d, ldx), float("nan"), dtype=torch.float64, device=DEV); dX[:, :n] = torch.from_numpy(np.array(X.T, order="C")).to(DEV)
    dU = torch.full((d, ldu), float("nan"), dtype=torch.float64, device=DEV); dU[:, :s] = torch.from_numpy(np.array(U.T, order="C")).to(DEV)
    rows, dpad = L.flgp_dev_anchor_rows(s), L.flgp_dev_anchor_dpad(d)
    dUt = torch.zeros(rows * dpad, dtype=torch.float64, device=DEV); duu = torch.zeros(rows, dtype=torch.float64, device=DEV)
    _lib.check(L.flgp_dev_anchor_prep(None, dU.data_ptr(), s, ldu, d, dUt.data_ptr(), duu.data_ptr()))
    d_w = torch.from_numpy(np.array(w)).to(DEV); d_P = torch.from_numpy(np.array(P)).to(DEV)
    d_cg = torch.from_numpy(np.array(cg)).to(DEV)
    d_mean = torch.full((groups * q + 1, ldm), float("nan"), dtype=torch.float64, device=DEV)
    d_var = torch.full((groups + 1, ldv), float("nan"), dtype=torch.float64, device=DEV)
    wb = L.flgp_dev_nystrom_predictor_workspace(n, s, groups, K, q, int(want_var))
    assert wb > 0
    work = torch.full((wb // 8 + 4,), float("nan"), dtype=torch.float64, device=DEV)       # four canary doubles behind the workspace
    rc = L.flgp_dev_nystrom_predictor_rows(None, dX.data_ptr(), n, ldx, d, dUt.data_ptr(), duu.data_ptr(), dU.data_ptr(), ldu, s,
                                           inv_c, d_w.data_ptr(), d_P.data_ptr(), ldp, groups, K, q, d_cg.data_ptr(),
                                           d_mean.data_ptr() if want_mean else None, ldm, d_var.data_ptr() if want_var else None, ldv,
                                           work.data_ptr(), wb)
    assert rc == 0, L.flgp_last_error().decode()
    torch.cuda.synchronize()
    mean, var = d_mean.cpu().numpy(), d_var.cpu().numpy()
    assert np.isnan(mean[:, n:]).all() and np.isnan(mean[groups * q:]).all()
    assert np.isnan(var[:, n:]).all() and np.isnan(var[groups:]).all()
    assert np.isnan(work[wb // 8:].cpu().numpy()).all()
    if not want_mean:
        assert np.isnan(mean).all()
    if not want_var:
        assert np.isnan(var).all()
    np.testing.assert_array_equal(d_P.cpu().numpy(), P)
    np.testing.assert_array_equal(dX[:, :n].cpu().numpy(), X.T); assert torch.isnan(dX[:, n:]).all()
    np.testing.assert_array_equal(d_w.cpu().numpy(), w)
    return mean[:groups * q, :n].T, var[:groups, :n].T


def reference(X, U, inv_c, w, P, cg, groups, K, q, dpad):
    """the long-double posterior and the forward bounds of the mean (n x groups q) and the variance (n x groups)"""
    n, s = X.shape[0], U.shape[0]
    wd = K + q
    mean, var = nnp.rows(X, U, inv_c, w, P, groups, K, q, cg, LD)
    Z = nnp.similarity(X, U, inv_c, LD)
    assert (Z.sum(1) > 1e-200).all()
    f = nnp.row_factor(Z, w, LD)
    Xl, Ul = np.abs(X).astype(LD), np.abs(U).astype(LD)
    S = (Xl * Xl).sum(1)[:, None] + 2 * (Xl @ Ul.T) + (Ul * Ul).sum(1)[None, :]
    eta = (LD(dpad + 4) * EPS * S * LD(inv_c)).max(1) + 3 * EPS
    M = f[:, None] * (Z @ np.abs(P[:, :groups * wd]).astype(LD))                       # n x groups (K + q)
    b = (3 * eta + LD(3 * s + 12) * EPS)[:, None] * M
    bm = np.hstack([b[:, g * wd + K:(g + 1) * wd] for g in range(groups)])
    bv = np.stack([(2 * M[:, g * wd:g * wd + K] * b[:, g * wd:g * wd + K] + b[:, g * wd:g * wd + K] ** 2).sum(1)
                   + LD(K + 8) * EPS * (M[:, g * wd:g * wd + K] ** 2).sum(1) + EPS * LD(cg[g]) for g in range(groups)], axis=1)
    return mean, var, bm, bv


CASES = nc.cases()


@pytest.mark.parametrize("c", CASES, ids=["n{n}-d{d}-s{s}-K{K}-q{q}-g{groups}".format(**c) for c in CASES])
def test_rows_against_the_long_double_restatement(c):
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    n, d, s, K, q, groups = (c[k] for k in ("n", "d", "s", "K", "q", "groups"))
    X, U, inv_c, w, P, ldp, cg = inputs(n, d, s, K, q, groups)
    ref_mean, ref_var, bm, bv = reference(X, U, inv_c, w, P, cg, groups, K, q, nc.dpad(d))
    assert np.abs(ref_mean).max() > 0 and float(bm.max()) <= 1e-9 * float(np.abs(ref_mean).max())
    got = {}
    for want_mean, want_var in nc.OUTPUTS:
        mean, var = got[want_mean, want_var] = run(X, U, inv_c, w, P, ldp, cg, groups, K, q, want_mean, want_var)
        rm = rv = 0.0
        if want_mean:
            rm = float((np.abs(mean.astype(LD) - ref_mean) / bm).max())
        if want_var:
            rv = float((np.abs(var.astype(LD) - ref_var) / bv).max())
            assert (var >= cg[None, :]).all()
        print(f"{nc.walk(**c, mean=want_mean, var=want_var)['route']} mean={want_mean} var={want_var}: "
              f"mean |d| / bound {rm:.3e}, var |d| / bound {rv:.3e}")
        assert rm <= 1.0 and rv <= 1.0
    np.testing.assert_array_equal(got[True, False][0], got[True, True][0])             # the mean without the variance
    np.testing.assert_array_equal(got[False, True][1], got[True, True][1])             # the variance without the mean


@pytest.mark.parametrize("d", [9, 40, 64, 70])
def test_bits_do_not_depend_on_the_call(d):
    """the same 513 rows: one call; blocks of 256; one row at a time; nystrom_dot_gemm 0 and 1 (d <= 64); T one group at a time"""
    L = _lib.lib()
    n, s, K, q, groups = nc.BIT_ROWS, 130, 130, 1, 3
    X, U, inv_c, w, P, ldp, cg = inputs(n, d, s, K, q, groups)
    want = run(X, U, inv_c, w, P, ldp, cg, groups, K, q)
    parts = [run(X[i0:i0 + 256], U, inv_c, w, P, ldp, cg, groups, K, q) for i0 in range(0, n, 256)]
    for k in (0, 1):
        np.testing.assert_array_equal(np.vstack([p[k] for p in parts]), want[k])
    for i in (0, 255, 256, 300, 512):
        one = run(X[i:i + 1], U, inv_c, w, P, ldp, cg, groups, K, q)
        np.testing.assert_array_equal(one[0][0], want[0][i]); np.testing.assert_array_equal(one[1][0], want[1][i])
    try:
        L.flgp_set_tuning(b"nystrom_predictor_t_mb", nc.T_MB_SMALL)
        small_t = run(X, U, inv_c, w, P, ldp, cg, groups, K, q)
    finally:
        L.flgp_set_tuning(b"nystrom_predictor_t_mb", 256)
    np.testing.assert_array_equal(small_t[0], want[0]); np.testing.assert_array_equal(small_t[1], want[1])
    if d <= 64:
        for knob in (0, 1):
            try:
                L.flgp_set_tuning(b"nystrom_dot_gemm", knob)
                other = run(X, U, inv_c, w, P, ldp, cg, groups, K, q)
                mean_only = run(X, U, inv_c, w, P, ldp, cg, groups, K, q, want_var=False)
            finally:
                L.flgp_set_tuning(b"nystrom_dot_gemm", -1)
            np.testing.assert_array_equal(other[0], want[0], err_msg=f"nystrom_dot_gemm={knob}")
            np.testing.assert_array_equal(other[1], want[1], err_msg=f"nystrom_dot_gemm={knob}")
            np.testing.assert_array_equal(mean_only[0], want[0], err_msg=f"nystrom_dot_gemm={knob}, mean alone")
    assert (want[1] >= cg[None, :]).all()
