"""GPU (-m gpu): the draws handle (include/flgp_hip.h) on the fits of tests/predictor_joint_fits.py: "lae" and
"se" models, regression (q = 3) and logit (3 groups), and one Nystrom bandwidth on both of its routes.

* P_draw from to_host is the restatement's fold (tests/np_predictor_draws.py) of the source's P and the handle's own normals(),
  bit for bit; the normals are flgp_amd/synth.py's within the bound of tests/test_gpu_predictor_draws_fold.py; draw t does not
  depend on S; dims and cg.
* the identity draws = mean + Z xi with Z = features(X), xi = normals() and the source handle's mean, the right side in long
  double.  Model handle: |d| <= (r + K + 4) u sum_a sum_k |A(i, a) P(j_a, g w + k) xi_k| + u |mean|, u = 2^-53: both sides are
  the same sum, reassociated.  Nystrom handle: with kappa_i = 3 eta_i + (3 s + 12) u, f-21's relative bound of one served
  column, the mean, every Z_k and the draw are each within kappa_i of their exact values on the absolute operand, and P_draw
  itself is a (K + 1)-term chain: |d| <= (2 kappa_i + (K + 2) u) f_i sum_j Z_ij (|P_mean(j)| + sum_k |P(j, k) xi_k|), taken
  times 1 + 2^-20 for the second-order terms.  Both routes (ncol <= 8 and ncol > 8) are held to it.
* consistency: 513 rows as one call, in blocks of 256, one at a time, through the host and the device entry; batch A served
  again inside a larger batch B; the source handle freed before the draws handle is used.
* the refusals that need live handles."""
import ctypes

import numpy as np
import pytest

import np_nystrom_predictor as nnp
import np_predictor_draws as npd
import predictor_draws_cases as pc
import predictor_joint_fits as pf
from flgp_amd import _lib, api

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LD, EPS = pf.LD, pf.EPS
SEED = 20260101
U24 = 24.0 * 2.0 ** -53


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()


def source(kind, shape, kernel, K):
    X = pf.case(shape)[0]
    model, pair, host = pf.fitted(shape, kernel)
    if kind == "regression":
        idx0, Y = pf.training(X, 60, 3, seed=K)
        return api.Predictor.regression(model, pair, Y, idx0, K, (pf.T, pf.NOISE), pf.SIGMA)
    idx0, Y, col, ts = pf.logit_problem(X, 60)
    return api.Predictor.logit(model, pair, idx0, K, ts, Y, col=col, sigma22=1e-3)


def check_handle(src, S, label):
    """dims, cg, P_draw against the fold of the device's own normals, the normals against synth; returns (draws handle, xi)"""
    groups, q, K = src.groups, src.q, src.K
    ncol = groups * q * S
    d = src.draws(S, SEED)
    assert d.dims == {"d": src.d, "s": src.s, "r": src.r, "K": K, "groups": 1, "q": ncol, "kind": "draws", "ldp": (ncol + 15) // 16 * 16}
    assert d.draw_shape == (groups, q, S)
    host = d.to_host()
    np.testing.assert_array_equal(host["cg"], [0.0])
    xi = d.normals()
    assert xi.shape == (K, ncol)
    np.testing.assert_array_equal(host["P"][:, :ncol], npd.fold(src.to_host()["P"], groups, K, q, S, xi), err_msg=label)
    assert (host["P"][:, ncol:] == 0.0).all()                                   # the padding columns
    ratio = (np.abs(xi - npd.normals(SEED, K, groups, q, S)) / (U24 * npd.radius(SEED, K, groups, q, S))).max()
    assert ratio <= 1.0, (label, ratio)
    return d, xi


@pytest.mark.parametrize("kind,shape,kernel,K", [("regression", "A", "lae", 20), ("regression", "A", "se", 12), ("logit", "A", "lae", 12),
                                                 ("logit", "A", "se", 20), ("regression", "As", "lae", 200)])
def test_model_draws_are_the_mean_plus_z_xi(kind, shape, kernel, K):
    src = source(kind, shape, kernel, K)
    groups, q, r = src.groups, src.q, src.r
    w = K + q
    Xn = pf.new_rows(shape, 130)
    idx, val = pf.model_ell_rows(shape, kernel, Xn)
    P = src.to_host()["P"]
    mean = src.apply(Xn, var=False)["mean"]
    Z = [src.features(Xn, group=g) for g in range(groups)]
    worst, kept = 0.0, {}
    for S in sorted({S for g_, q_, S in pc.HANDLE_DRAWS if (g_, q_) == (groups, q)} | {3}):
        label = f"{kind} {shape} {kernel} K={K} S={S}"
        d, xi = check_handle(src, S, label)
        f = d.apply(Xn)
        assert f.shape == (130, groups, q, S)
        _lib.lib().flgp_set_tuning(b"predictor_cols_tile_min", 1)                # the tile kernel at this width: the same bits
        try:
            np.testing.assert_array_equal(d.apply(Xn), f)
        finally:
            _lib.lib().flgp_set_tuning(b"predictor_cols_tile_min", pc.TILE_MIN)
        kept[S] = (d.to_host()["P"], f)
        absAP = np.abs(val)[:, :, None] * np.abs(P[idx])                        # n x r x ldp: |A(i, a) P(j_a, :)|
        for g in range(groups):
            for c in range(q):
                for t in range(S):
                    x = xi[:, (g * q + c) * S + t]
                    want = mean[:, g * q + c].astype(LD) + Z[g].astype(LD) @ x.astype(LD)
                    bound = (r + K + 4) * EPS * (absAP[:, :, g * w:g * w + K].astype(LD) @ np.abs(x).astype(LD)).sum(1) \
                        + EPS * np.abs(mean[:, g * q + c]).astype(LD)
                    worst = max(worst, float((np.abs(f[:, g, c, t].astype(LD) - want) / bound).max()))
        d.free()
    print(f"{kind} {shape} {kernel} K={K}: largest |draws - (mean + Z xi)| / bound = {worst:.3f}")
    assert worst <= 1.0
    # draw t does not depend on S: P_draw and the served values
    sizes = sorted(kept)
    big = sizes[-1]
    for S in sizes[:-1]:
        for gc in range(groups * q):
            np.testing.assert_array_equal(kept[S][0][:, gc * S:(gc + 1) * S], kept[big][0][:, gc * big:gc * big + S])
        np.testing.assert_array_equal(kept[S][1], kept[big][1][..., :S])
    src.free()


@pytest.mark.parametrize("kind", ["regression", "logit"])
def test_nystrom_draws_on_both_routes(kind):
    i = 1
    X, Ua, X2 = pf.ny_cloud()
    grid, pairs = pf.ny_fitted()
    n, d, s, K = pf.NY
    if kind == "regression":
        idx0, Y = pf.training(X, 60, 3, seed=K)
        src = api.Predictor.nystrom_regression(grid, i, pairs[i], Y, idx0, K, (pf.T, pf.NOISE), pf.SIGMA)
    else:
        idx0, Y, col, ts = pf.logit_problem(X, 60)
        src = api.Predictor.nystrom_logit(grid, i, pairs[i], idx0, K, ts, Y, col=col, sigma22=1e-3)
    groups, q = src.groups, src.q
    w = K + q
    Xn = np.asfortranarray(X2[:130])
    P = src.to_host()["P"]
    mean = src.apply(Xn, var=False)["mean"]
    Z = [src.features(Xn, group=g) for g in range(groups)]
    inv_c = 1.0 / (pf.A2S[i] * grid.distances_mean)
    wv = 1 / (nnp.similarity(Ua, Ua, inv_c, LD).sum(1) + LD(1e-9))
    Zs = nnp.similarity(Xn, Ua, inv_c, LD)
    fz = nnp.row_factor(Zs, wv, LD)[:, None] * Zs                               # f_i Z_ij
    Xl, Ul = np.abs(Xn).astype(LD), np.abs(Ua).astype(LD)
    Sx = (Xl * Xl).sum(1)[:, None] + 2 * (Xl @ Ul.T) + (Ul * Ul).sum(1)[None, :]
    eta = (LD(_lib.lib().flgp_dev_anchor_dpad(d) + 4) * EPS * Sx * LD(inv_c)).max(1) + 3 * EPS
    kappa = 3 * eta + LD(3 * s + 12) * EPS
    worst, routes = 0.0, set()
    for S in (2, 5, 30):
        label = f"nystrom {kind} S={S}"
        dh, xi = check_handle(src, S, label)
        routes.add(pc.nystrom_route("draws", groups * q * S))
        f = dh.apply(Xn)
        for g in range(groups):
            for c in range(q):
                for t in range(S):
                    x = xi[:, (g * q + c) * S + t]
                    want = mean[:, g * q + c].astype(LD) + Z[g].astype(LD) @ x.astype(LD)
                    operand = np.abs(P[:, g * w + K + c]).astype(LD) + np.abs(P[:, g * w:g * w + K]).astype(LD) @ np.abs(x).astype(LD)
                    bound = (2 * kappa + LD(K + 2) * EPS) * (fz @ operand) * (1 + LD(2.0) ** -20)
                    worst = max(worst, float((np.abs(f[:, g, c, t].astype(LD) - want) / bound).max()))
        # a row's bits on this handle do not depend on the call
        np.testing.assert_array_equal(dh.apply(Xn[77:78])[0], f[77])
        dh.free()
    assert routes == {"mean", "cols"}
    print(f"nystrom {kind}: largest |draws - (mean + Z xi)| / bound = {worst:.3f}")
    assert worst <= 1.0
    src.free()


@pytest.mark.parametrize("where", ["model", "nystrom-mean", "nystrom-cols"])
def test_draws_are_functions(where):
    import torch
    if where == "model":
        src = source("regression", "A", "lae", 20)
        X3 = pf.new_rows("A", pc.BIT_ROWS, seed=99)
        S = 30
    else:
        X, Ua, X2 = pf.ny_cloud()
        grid, pairs = pf.ny_fitted()
        idx0, Y = pf.training(X, 60, 3, seed=7)
        src = api.Predictor.nystrom_regression(grid, 0, pairs[0], Y, idx0, pf.NY[3], (pf.T, pf.NOISE), pf.SIGMA)
        X3 = np.asfortranarray(X2[:pc.BIT_ROWS])
        S = 2 if where == "nystrom-mean" else 30
    d_ = X3.shape[1]
    dh = src.draws(S, SEED)
    src.free()                                                                  # the draws handle does not borrow its source
    ncol = dh.q
    L = _lib.lib()
    want = dh.apply(X3)
    L.flgp_set_tuning(b"model_extend_block", 256)
    try:
        small = dh.apply(X3)
        n_new, ldx, ldm = pc.BIT_ROWS, pc.BIT_ROWS + 3, pc.BIT_ROWS + 5         # the device-pointer entry on padded buffers
        dX = torch.full((d_, ldx), float("nan"), dtype=torch.float64, device=DEV)
        dX[:, :n_new] = torch.from_numpy(np.ascontiguousarray(X3.T)).to(DEV)
        dm = torch.full((ncol + 1, ldm), float("nan"), dtype=torch.float64, device=DEV)
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(L.flgp_dev_predictor_apply(st, dh._h, dX.data_ptr(), n_new, ldx, dm.data_ptr(), ldm, None, 0))
        torch.cuda.synchronize()
    finally:
        L.flgp_set_tuning(b"model_extend_block", 1 << 20)
    np.testing.assert_array_equal(small, want)
    L.flgp_set_tuning(b"predictor_cols_tile_min", 1)                            # (a model handle: the tile kernel at this width)
    try:
        np.testing.assert_array_equal(dh.apply(X3), want)
    finally:
        L.flgp_set_tuning(b"predictor_cols_tile_min", pc.TILE_MIN)
    dm = dm.cpu().numpy()
    np.testing.assert_array_equal(dm[:ncol, :n_new].T, want.reshape(n_new, ncol))
    assert np.isnan(dm[ncol]).all() and np.isnan(dm[:, n_new:]).all()
    for i in (0, 255, 256, 300, 512):
        np.testing.assert_array_equal(dh.apply(X3[i:i + 1])[0], want[i])
    # batch A served again inside a larger batch B, at other positions
    A = X3[40:140]
    B = np.asfortranarray(np.vstack([X3[300:400], A, X3[:17]]))
    np.testing.assert_array_equal(dh.apply(B)[100:200], dh.apply(A))
    np.testing.assert_array_equal(dh.apply(A), want[40:140])
    dh.free()


def test_refusals_that_need_live_handles():
    X = pf.case("A")[0]
    model, pair, host = pf.fitted("A")
    idx0, Y, col, ts = pf.logit_problem(X, 60)
    pred = api.Predictor.logit(model, pair, idx0, 12, ts, Y, col=col)
    L = _lib.lib()

    def raw(h, S):
        out = ctypes.c_void_p(1)
        rc_ = L.flgp_predictor_draws_create(h, S, SEED, ctypes.byref(out))
        return rc_, out.value, L.flgp_last_error().decode()

    assert raw(pred._h, 0) == (-1, None, "predictor_draws: need S >= 1 (S=0)")
    assert raw(pred._h, -3) == (-1, None, "predictor_draws: need S >= 1 (S=-3)")
    assert raw(pred._h, 2 ** 30) == (-1, None, f"predictor_draws: groups q S = {3 * 2 ** 30} columns overflow an int")
    draws = pred.draws(2, SEED)
    pg = api.Predictor.pg(model, pair, idx0, 12, ts, Y, 1e-2, col=col, seed=3, N_sample=3)
    # the kind comes before S
    assert raw(draws._h, 0) == (-1, None, "predictor_draws: a handle of kind 3 has no covariance operand")
    assert raw(pg._h, 0) == (-1, None, "predictor_draws: a handle of kind 2 has no covariance operand")
    xi = np.zeros((12, 6), order="F")
    assert L.flgp_predictor_draws_normals(pred._h, xi.ctypes.data) == -1
    assert L.flgp_last_error().decode() == "predictor_draws_normals: the handle is not a draws one (kind 1)"
    # var on a draws handle
    Xa = np.asfortranarray(X[:9]); m_ = np.zeros((9, 6), order="F"); v_ = np.zeros(9)
    assert L.flgp_predictor_apply(draws._h, Xa.ctypes.data, 9, m_.ctypes.data, v_.ctypes.data) == -1
    assert L.flgp_last_error().decode() == "predictor_apply: a draws handle has no variance"
    assert L.flgp_dev_predictor_apply(None, draws._h, FAKE, 9, 9, FAKE, 9, FAKE, 9) == -1
    assert L.flgp_last_error().decode() == "predictor_apply: a draws handle has no variance"
    with pytest.raises(api.FlgpError, match="predictor_pg_apply: the handle is not a Polya-Gamma one"):
        draws.predict(Xa)
    # a NaN in X is the input check's refusal, and the handle stays usable
    good = draws.apply(Xa)
    bad = np.array(Xa, order="F"); bad[4, 1] = np.nan
    with pytest.raises(api.FlgpError, match="points"):
        draws.apply(bad)
    np.testing.assert_array_equal(draws.apply(Xa), good)
    with pytest.raises(ValueError, match="columns"):
        draws.apply(np.zeros((4, 4)))
    draws.free(); pg.free(); pred.free()
    with pytest.raises(ValueError, match="freed"):
        draws.apply(Xa)


FAKE = 8               # a non-null pointer: the refusal comes before it is looked at
