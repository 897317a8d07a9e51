"""GPU (-m gpu): flgp_predictor_features and flgp_predictor_covariance (include/flgp_hip.h) on the fits of
tests/predictor_joint_fits.py: "lae" and "se" models and one Nystrom bandwidth, regression and logit, m = 10 <= K = 12 and
m = 60 > K.

* covariance against the dense route the reference's algebra gives, in long double: u the rows of model.extend / grid.extend on
  the fit rows stacked on 40 new rows, Lambda = exp(-t (1 - values)), C(A, B) = U_A Lambda U_B^T and
    regression  Sigma = C(a, b) - C(a, 1) (C(1, 1) + (noise + sigma) I)^-1 C(1, b)
    logit       Sigma = C(a, b) - C(a, 1) W^1/2 B^-1 W^1/2 C(1, b) at the restatement's mode, sigma11 on C(1, 1),
  judged by the project's own variance tolerances -- regression_posterior_cases.atol_var, np_logit_posterior.tolerances -- taken
  with the block's largest reference diagonal (cg included) and largest prior: an off-diagonal entry of the same factor is
  bounded by the diagonals through Cauchy-Schwarz.  |d| / bound is printed (recorded in DESIGN f-23).
* Xb = None: the block equals its transpose bit for bit and its diagonal is >= 0; diag_term adds cg.
* diag(covariance) + cg against apply's var: |d| <= (K + 8) 2^-53 sum_k z_k^2 -- the same squares, another order.
* features: on a model handle the cols restatement on the model's ELL rows, bit for bit; on the Nystrom handle the long-double
  restatement within f-21's b_ik = (3 eta_i + (3 s + 12) u) M_ik, M_ik = f_i sum_j Z_ij |P(j, k)|.
* 513 rows across the block seam (model_extend_block = 256 against the default): features from host and device rows and a
  513 x 300 covariance block bit for bit, on a model and a Nystrom handle; a NaN behind the first block is refused and the
  handle stays usable.
* the refusals that need live handles."""
import numpy as np
import pytest

import np_logit_posterior as nlp
import np_nystrom_predictor as nnp
import np_predictor_draws as npd
import predictor_joint_fits as pf
import regression_posterior_cases as rc
from flgp_amd import _lib, api

pytestmark = pytest.mark.gpu
K12, NEW = 12, 40
LD, EPS = pf.LD, pf.EPS
U53 = 2.0 ** -53


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()


def check_block(pred, g, Xa, ref, bound, cg, label, K):
    """the symmetric block and two rectangular ones against ref (na x na, long double); returns the largest |d| / bound"""
    C = pred.covariance(Xa, group=g)
    assert C.shape == ref.shape and C.flags.f_contiguous
    np.testing.assert_array_equal(C, C.T)                                       # bit for bit
    assert (np.diag(C) >= 0.0).all()
    worst = float(np.abs(C.astype(LD) - ref).max()) / bound
    rect = pred.covariance(Xa[:25], Xa[10:], group=g)
    worst = max(worst, float(np.abs(rect.astype(LD) - ref[:25, 10:]).max()) / bound)
    one = pred.covariance(Xa[3:4], Xa, group=g)
    worst = max(worst, float(np.abs(one.astype(LD) - ref[3:4]).max()) / bound)
    print(f"{label}: covariance |d| / bound = {worst:.3e} (bound {bound:.3e}, largest diagonal {float(np.diag(ref).max()):.3e})")
    assert worst <= 1.0
    # the diagonal term, and the diagonal against apply's variance
    Cd = pred.covariance(Xa, group=g, diag_term=True)
    off = ~np.eye(C.shape[0], dtype=bool)
    np.testing.assert_array_equal(Cd[off], C[off]); np.testing.assert_array_equal(np.diag(Cd), np.diag(C) + cg)
    Z = pred.features(Xa, group=g)
    assert Z.shape == (Xa.shape[0], K)
    var = pred.apply(Xa)["var"][:, g]
    sq = (Z * Z).sum(1)
    dv = np.abs((np.diag(C).astype(LD) + LD(cg)) - var.astype(LD))              # the sum on this side in long double
    ratio = float((dv / (LD(K + 8) * EPS * sq.astype(LD))).max())
    print(f"{label}: diag + cg against var, largest |d| / ((K + 8) u sum z^2) = {ratio:.3f}")
    assert ratio <= 1.0
    return worst


@pytest.mark.parametrize("m", [10, 60])
@pytest.mark.parametrize("kernel", ["lae", "se"])
def test_model_regression_covariance(kernel, m):
    X = pf.case("A")[0]
    model, pair, host = pf.fitted("A", kernel)
    idx0, Y = pf.training(X, m, 3, seed=K12 + m)
    Xa = pf.new_rows("A", NEW)
    U = model.extend(np.vstack([X[idx0], Xa])).vectors
    np.testing.assert_array_equal(U[:m], host.vectors[idx0])                    # fit rows come back bit for bit
    c = pf.NOISE + pf.SIGMA
    ref, prior = pf.regression_cov(host.values, U[:m], U[m:], U[m:], K12, pf.T, c)
    bound = rc.atol_var(dict(var=np.diag(ref).astype(np.float64) + c, prior=prior, m=m, c=c))
    pred = api.Predictor.regression(model, pair, Y, idx0, K12, (pf.T, pf.NOISE), pf.SIGMA)
    check_block(pred, 0, Xa, ref, bound, c, f"regression {kernel} m={m}", K12)
    pred.free()


@pytest.mark.parametrize("m", [10, 60])
@pytest.mark.parametrize("kernel", ["lae", "se"])
def test_model_logit_covariance(kernel, m):
    X = pf.case("A")[0]
    model, pair, host = pf.fitted("A", kernel)
    idx0, Y, col, ts = pf.logit_problem(X, m)
    Xa = pf.new_rows("A", NEW)
    U = model.extend(np.vstack([X[idx0], Xa])).vectors
    sigma11, sigma22 = 0.05, 1e-3
    pred = api.Predictor.logit(model, pair, idx0, K12, ts, Y, col=col, sigma11=sigma11, sigma22=sigma22, tol=pf.NEWTON_TOL)
    for b in range(3):
        ref, prior = pf.logit_cov(host.values, U[:m], U[m:], U[m:], K12, ts[b], Y[:, col[b]], sigma11)
        bound = nlp.tolerances(np.zeros(1), np.diag(ref).astype(np.float64) + sigma22, np.array([prior + sigma22]), m)[1]
        check_block(pred, b, Xa, ref, bound, sigma22, f"logit {kernel} m={m} problem {b}", K12)
    pred.free()


@pytest.mark.parametrize("m", [10, 60])
def test_nystrom_covariance(m):
    i = 1
    X, Ua, X2 = pf.ny_cloud()
    grid, pairs = pf.ny_fitted()
    K = pf.NY[3]
    Xa = np.asfortranarray(X2[:NEW])
    idx0, Y = pf.training(X, m, 3, seed=K + m)
    both = grid.extend(i, np.vstack([X[idx0], Xa]))
    U, values = both.vectors, both.values
    c = pf.NOISE + pf.SIGMA
    ref, prior = pf.regression_cov(values, U[:m], U[m:], U[m:], K, pf.T, c)
    bound = rc.atol_var(dict(var=np.diag(ref).astype(np.float64) + c, prior=prior, m=m, c=c))
    pred = api.Predictor.nystrom_regression(grid, i, pairs[i], Y, idx0, K, (pf.T, pf.NOISE), pf.SIGMA)
    check_block(pred, 0, Xa, ref, bound, c, f"nystrom regression m={m}", K)
    pred.free()
    idx0, Yb, col, ts = pf.logit_problem(X, m)
    both = grid.extend(i, np.vstack([X[idx0], Xa]))
    U = both.vectors
    sigma11, sigma22 = 0.05, 1e-3
    pred = api.Predictor.nystrom_logit(grid, i, pairs[i], idx0, K, ts, Yb, col=col, sigma11=sigma11, sigma22=sigma22, tol=pf.NEWTON_TOL)
    for b in (0, 2):
        ref, prior = pf.logit_cov(values, U[:m], U[m:], U[m:], K, ts[b], Yb[:, col[b]], sigma11)
        bound = nlp.tolerances(np.zeros(1), np.diag(ref).astype(np.float64) + sigma22, np.array([prior + sigma22]), m)[1]
        check_block(pred, b, Xa, ref, bound, sigma22, f"nystrom logit m={m} problem {b}", K)
    pred.free()


@pytest.mark.parametrize("shape,K", [("A", 12), ("A", 20), ("As", 200)])
def test_model_features_are_the_cols_restatement_bit_for_bit(shape, K):
    X = pf.case(shape)[0]
    for kernel in ("lae", "se"):
        model, pair, host = pf.fitted(shape, kernel)
        idx0, Y, col, ts = pf.logit_problem(X, 60)
        pred = api.Predictor.logit(model, pair, idx0, K, ts, Y, col=col, sigma22=1e-3)
        Xn = pf.new_rows(shape, 257)
        idx, val = pf.model_ell_rows(shape, kernel, Xn)
        P = pred.to_host()["P"]
        for g in range(3):
            Z = pred.features(Xn, group=g)
            np.testing.assert_array_equal(Z, npd.cols(idx, val, P, g * (K + 1), K), err_msg=f"{shape} {kernel} K={K} group {g}")
            # K < 512 columns go to predictor_pg_rows_kernel at the default knob: the tile kernel gives the same bits
            _lib.lib().flgp_set_tuning(b"predictor_cols_tile_min", 1)
            try:
                np.testing.assert_array_equal(pred.features(Xn, group=g), Z)
            finally:
                _lib.lib().flgp_set_tuning(b"predictor_cols_tile_min", 512)
        np.testing.assert_array_equal(pred.features(Xn[100:101], group=1)[0], pred.features(Xn, group=1)[100])
        pred.free()


def test_nystrom_features_against_the_long_double_restatement():
    i = 0
    X, Ua, X2 = pf.ny_cloud()
    grid, pairs = pf.ny_fitted()
    n, d, s, K = pf.NY
    idx0, Y = pf.training(X, 60, 3, seed=5)
    pred = api.Predictor.nystrom_regression(grid, i, pairs[i], Y, idx0, K, (pf.T, pf.NOISE), pf.SIGMA)
    Xn = np.asfortranarray(X2[:257])
    Z = pred.features(Xn)
    P = pred.to_host()["P"][:, :K]
    inv_c = 1.0 / (pf.A2S[i] * grid.distances_mean)
    w = 1 / (nnp.similarity(Ua, Ua, inv_c, LD).sum(1) + LD(1e-9))
    Zs = nnp.similarity(Xn, Ua, inv_c, LD)
    f = nnp.row_factor(Zs, w, LD)
    ref = f[:, None] * (Zs @ P.astype(LD))
    Xl, Ul = np.abs(Xn).astype(LD), np.abs(Ua).astype(LD)
    S = (Xl * Xl).sum(1)[:, None] + 2 * (Xl @ Ul.T) + (Ul * Ul).sum(1)[None, :]
    dpad = _lib.lib().flgp_dev_anchor_dpad(d)
    eta = (LD(dpad + 4) * EPS * S * LD(inv_c)).max(1) + 3 * EPS
    M = f[:, None] * (Zs @ np.abs(P).astype(LD))
    b = (3 * eta + LD(3 * s + 12) * EPS)[:, None] * M
    ratio = float((np.abs(Z.astype(LD) - ref) / b).max())
    print(f"nystrom features: largest |d| / b_ik = {ratio:.3f}")
    assert np.abs(ref).max() > 0 and ratio <= 1.0
    np.testing.assert_array_equal(pred.features(Xn[100:101])[0], Z[100])
    pred.free()


SEAM = 513                                                                      # two blocks of 256 rows and a block of one


def seam_handle(which):
    """(a regression handle, 513 unseen rows): over the "lae" model of shape A, or over bandwidth 1 of the Nystrom grid"""
    if which == "model":
        X = pf.case("A")[0]
        model, pair, host = pf.fitted("A")
        idx0, Y = pf.training(X, 60, 3, seed=7)
        return api.Predictor.regression(model, pair, Y, idx0, K12, (pf.T, pf.NOISE), pf.SIGMA), pf.new_rows("A", SEAM)
    X, Ua, X2 = pf.ny_cloud()
    grid, pairs = pf.ny_fitted()
    idx0, Y = pf.training(X, 60, 3, seed=7)
    return api.Predictor.nystrom_regression(grid, 1, pairs[1], Y, idx0, pf.NY[3], (pf.T, pf.NOISE), pf.SIGMA), np.asfortranarray(X2[:SEAM])


def dev_features(pred, Xn, ldx, ldz):
    """flgp_dev_predictor_features on padded, NaN-filled buffers with a spare output column: the (K + 1) x ldz buffer as it is left"""
    import torch
    n, d = Xn.shape
    dX = torch.full((d, ldx), float("nan"), dtype=torch.float64, device=pf.DEV)
    dX[:, :n] = torch.from_numpy(np.ascontiguousarray(Xn.T)).to(pf.DEV)
    dZ = torch.full((pred.K + 1, ldz), float("nan"), dtype=torch.float64, device=pf.DEV)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().flgp_dev_predictor_features(st, pred._h, 0, dX.data_ptr(), n, ldx, dZ.data_ptr(), ldz))
    torch.cuda.synchronize()
    return dZ.cpu().numpy()


@pytest.mark.parametrize("which", ["model", "nystrom"])
def test_features_and_covariance_bits_across_a_block_seam(which):
    """513 rows at model_extend_block = 256 are three blocks, at the default one: features (host rows and device rows) and a
    513 x 300 covariance block give the same bits either way.  On the model handle each element is one chain over a row's own
    weights; on the Nystrom handle a row's Z, f and T chains do not see the block either (apply's are asserted equal at the
    two block sizes in tests/test_gpu_nystrom_predictor.py)."""
    pred, Xn = seam_handle(which)
    K = pred.K
    Xb = np.asfortranarray(Xn[200:500])
    L = _lib.lib()
    want = {"Z": pred.features(Xn), "dev": dev_features(pred, Xn, 516, 518), "C": pred.covariance(Xn, Xb)}
    L.flgp_set_tuning(b"model_extend_block", 256)
    try:
        got = {"Z": pred.features(Xn), "dev": dev_features(pred, Xn, 516, 518), "C": pred.covariance(Xn, Xb)}
    finally:
        L.flgp_set_tuning(b"model_extend_block", 1 << 20)
    assert want["Z"].shape == (SEAM, K) and want["C"].shape == (SEAM, 300) and np.isfinite(want["Z"]).all() and np.abs(want["Z"]).max() > 0
    for key in ("Z", "C"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{which} {key}")
    for dZ in (want["dev"], got["dev"]):
        np.testing.assert_array_equal(dZ[:K, :SEAM].T, want["Z"], err_msg=f"{which} device entry")
        assert np.isnan(dZ[K]).all() and np.isnan(dZ[:, SEAM:]).all()           # the spare column and the padding rows
    pred.free()


def test_a_non_finite_point_behind_the_first_block_is_refused():
    """a NaN in row 300 of 513 at model_extend_block = 256: the second block is the one that is refused, after the first one's
    work was queued; the handle gives its unchanged bits on clean rows straight after"""
    L = _lib.lib()
    for which in ("model", "nystrom"):
        pred, Xn = seam_handle(which)
        bad = np.array(Xn, order="F"); bad[300, 1] = np.nan
        want = pred.apply(Xn)
        Z = pred.features(Xn) if which == "model" else None
        L.flgp_set_tuning(b"model_extend_block", 256)
        try:
            with pytest.raises(api.FlgpError, match="points"):
                pred.apply(bad)
            got = pred.apply(Xn)
            if which == "model":
                with pytest.raises(api.FlgpError, match="points"):
                    pred.features(bad)
                np.testing.assert_array_equal(pred.features(Xn), Z)
        finally:
            L.flgp_set_tuning(b"model_extend_block", 1 << 20)
        for key in ("mean", "var"):
            np.testing.assert_array_equal(got[key], want[key], err_msg=f"{which} {key}")
        pred.free()


def test_refusals_that_need_live_handles():
    X = pf.case("A")[0]
    model, pair, host = pf.fitted("A")
    idx0, Y, col, ts = pf.logit_problem(X, 60)
    pred = api.Predictor.logit(model, pair, idx0, K12, ts, Y, col=col)
    L = _lib.lib()
    Xa = np.asfortranarray(X[:9]); Z = np.zeros((9, K12), order="F"); C = np.zeros((9, 9), order="F")
    for g in (-1, 3):
        assert L.flgp_predictor_features(pred._h, g, Xa.ctypes.data, 9, Z.ctypes.data) == -1
        assert L.flgp_last_error().decode() == f"predictor_features: group {g} outside 0..2"
        assert L.flgp_predictor_covariance(pred._h, g, Xa.ctypes.data, 9, None, 0, C.ctypes.data) == -1
        assert L.flgp_last_error().decode() == f"predictor_covariance: group {g} outside 0..2"
    good = pred.covariance(Xa, group=1)
    bad = np.array(Xa, order="F"); bad[4, 1] = np.nan
    for call in (lambda: pred.features(bad), lambda: pred.covariance(bad), lambda: pred.covariance(Xa, bad)):
        with pytest.raises(api.FlgpError, match="points"):
            call()
    np.testing.assert_array_equal(pred.covariance(Xa, group=1), good)            # the handle stays usable
    draws = pred.draws(2, 5)
    pg = api.Predictor.pg(model, pair, idx0, K12, ts, Y, 1e-2, col=col, seed=3, N_sample=3)
    for other, kind in ((draws, 3), (pg, 2)):
        assert L.flgp_predictor_features(other._h, 0, Xa.ctypes.data, 9, Z.ctypes.data) == -1
        assert L.flgp_last_error().decode() == f"predictor_features: a handle of kind {kind} has no covariance operand"
        assert L.flgp_predictor_covariance(other._h, 0, Xa.ctypes.data, 9, None, 0, C.ctypes.data) == -1
        assert L.flgp_last_error().decode() == f"predictor_covariance: a handle of kind {kind} has no covariance operand"
    draws.free(); pg.free(); pred.free()
