"""GPU (-m gpu): flgp_predictor_update / flgp_dev_predictor_update (include/flgp_hip.h) on the fits of
tests/predictor_joint_fits.py: "A" (K = 20) and "As" (K = 200), "lae" and "se", at T, NOISE, SIGMA.  The newly labelled rows are
fit rows outside idx0: the model reproduces fit rows bit for bit, so Predictor.regression on the stacked index set is the
device-side comparator and needs no extension.

* Against long double: h0 on m0 in {12, 60} rows, q in {1, 3}, updated with n_b in {1, 7, 300} rows; the mean and the variance of
  500 unseen rows and a 40 x 40 covariance block against the dense conditioning
    mean = C(u, 1) (C(1, 1) + diag d)^-1 Y,   Sigma = C(u, u) - C(u, 1) (C(1, 1) + diag d)^-1 C(1, u),   d_i = noise_i + sigma
  over the m0 + n_b stacked rows (prior_block and ld_spd_solve of tests/predictor_joint_fits.py: regression_cov with a diagonal
  noise), within atol_mean / atol_var of tests/regression_posterior_cases.py, the forms f-20 holds the fresh handle to.  The
  fresh handle on the stacked set is held to the same bound in the same test; both ratios are printed (recorded in DESIGN f-24).
* Per-row noise on the new rows: the mean also against the fresh "different" create with noise [NOISE x m0 ; noise_new] (both
  within atol_mean of the reference, so within twice that of each other).  The variance goes against long double only: the
  fresh "different" handle's variance is at noise[0] by design (f-20), so it is not the comparator.
* Chained updates: update(A) then update(B), update(A u B) and the fresh create agree within the bound.
* Invariants: var' >= cg bit for bit; var' <= var + (K + 8) 2^-53 sum_k z_k^2 (the squares shrink: z' = L^-1 z with M >= I; the
  slack is the rounding of the two sums of K squares); to_host of h0 has the same bits before and after; the updated handle
  works after h0 is freed; features, covariance and draws run on it.
* The same bits under model_extend_block in {256, 1 << 20} and from the host and the device entry, on 2500 rows (ten chunks: ten
  blocks of one chunk against one block).
* The live refusals: logit, PG and draws handles, a Nystrom handle, a "different" handle, a bad noise length, a non-finite Y or
  noise, noise + sigma <= 0, a NaN in X (h stays usable)."""
import ctypes
import functools

import numpy as np
import pytest

import predictor_joint_fits as pf
import regression_posterior_cases as rc
from flgp_amd import _lib, api

pytestmark = pytest.mark.gpu
LD, EPS = pf.LD, pf.EPS
UNSEEN, NCOV = 500, 40
FITS = [("A", "lae"), ("A", "se"), ("As", "lae"), ("As", "se")]


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()


def labelled(shape, m0, n_b, q, seed):
    """idx0 (m0 rows), the n_b new rows (fit rows outside idx0) and the responses of both"""
    X = pf.case(shape)[0]
    rng = np.random.default_rng(seed)
    rows = rng.permutation(X.shape[0])[:m0 + n_b].astype(np.int32)
    Y = np.asfortranarray(np.sin(2.0 * X[rows, :1] + np.arange(q)[None, :]) + 0.1 * rng.normal(size=(m0 + n_b, q)))
    return rows[:m0], rows[m0:], Y


@functools.lru_cache(maxsize=None)
def unseen(shape, kernel):
    """(the 500 unseen rows, their eigenvector rows under the model)"""
    Xu = pf.new_rows(shape, UNSEEN)
    U = pf.fitted(shape, kernel)[0].extend(Xu).vectors
    Xu.setflags(write=False); U.setflags(write=False)
    return Xu, U


def dense_reference(values, U1, d, Y, Uu, K):
    """the conditioning on the stacked rows in long double: mean (500 x q), latent variance (500), covariance block (40 x 40),
    and the largest prior diagonal of the unseen rows"""
    q = Y.shape[1]
    C1u = pf.prior_block(values, U1, Uu, K, pf.T)
    A = pf.prior_block(values, U1, U1, K, pf.T) + np.diag(np.asarray(d, dtype=LD))
    sol = pf.ld_spd_solve(A, np.hstack([np.asarray(Y, dtype=LD), C1u]))
    lam = np.exp(-LD(pf.T) * (1 - np.asarray(values[:K]).astype(LD)))
    prior = ((np.asarray(Uu)[:, :K].astype(LD) ** 2) * lam).sum(1)
    mean = C1u.T @ sol[:, :q]
    var = prior - (C1u * sol[:, q:]).sum(0)
    cov = pf.prior_block(values, Uu[:NCOV], Uu[:NCOV], K, pf.T) - C1u[:, :NCOV].T @ sol[:, q:q + NCOV]
    return mean, var, cov, float(prior.max())


def judge(pred, Xu, ref, m, c, label):
    """the largest |d| / bound of the mean, the variance and the covariance block; asserts all three"""
    mean, var, cov, prior = ref
    got = pred.apply(Xu)
    b_mean = rc.atol_mean(mean.astype(np.float64))
    b_var = rc.atol_var(dict(var=var.astype(np.float64) + c, prior=prior, m=m, c=c))
    r_mean = float(np.abs(got["mean"].astype(LD) - mean).max()) / b_mean
    r_var = float(np.abs(got["var"][:, 0].astype(LD) - (var + LD(c))).max()) / b_var
    C = pred.covariance(Xu[:NCOV])
    b_cov = rc.atol_var(dict(var=np.diag(cov).astype(np.float64) + c, prior=prior, m=m, c=c))
    r_cov = float(np.abs(C.astype(LD) - cov).max()) / b_cov
    print(f"{label}: |d| / bound  mean {r_mean:.3e}  var {r_var:.3e}  cov {r_cov:.3e}")
    assert r_mean <= 1.0 and r_var <= 1.0 and r_cov <= 1.0, label
    return got


@pytest.mark.parametrize("q", [1, 3])
@pytest.mark.parametrize("m0", [12, 60])
@pytest.mark.parametrize("shape,kernel", FITS)
def test_against_long_double(shape, kernel, m0, q):
    K = pf.SHAPES[shape][4]
    X = pf.case(shape)[0]
    model, pair, host = pf.fitted(shape, kernel)
    Xu, Uu = unseen(shape, kernel)
    c = pf.NOISE + pf.SIGMA
    for n_b in (1, 7, 300):
        idx0, idxb, Y = labelled(shape, m0, n_b, q, seed=1000 * m0 + 10 * n_b + q)
        rows = np.r_[idx0, idxb]
        ref = dense_reference(host.values, host.vectors[rows], np.full(m0 + n_b, c), Y, Uu, K)
        h0 = api.Predictor.regression(model, pair, Y[:m0], idx0, K, (pf.T, pf.NOISE), pf.SIGMA)
        h1 = h0.update(X[idxb], Y[m0:])
        fresh = api.Predictor.regression(model, pair, Y, rows, K, (pf.T, pf.NOISE), pf.SIGMA)
        assert h1.kind == "regression" and h1.dims == h0.dims
        label = f"{shape} {kernel} m0={m0} q={q} n_b={n_b}"
        judge(h1, Xu, ref, m0 + n_b, c, label + " updated")
        judge(fresh, Xu, ref, m0 + n_b, c, label + " fresh")
        for h in (h0, h1, fresh):
            h.free()


@pytest.mark.parametrize("shape,kernel", [("A", "lae"), ("As", "se")])
def test_per_row_noise_on_the_new_rows(shape, kernel):
    K = pf.SHAPES[shape][4]
    X = pf.case(shape)[0]
    model, pair, host = pf.fitted(shape, kernel)
    Xu, Uu = unseen(shape, kernel)
    m0, n_b, q = 60, 45, 3
    idx0, idxb, Y = labelled(shape, m0, n_b, q, seed=77)
    rows = np.r_[idx0, idxb]
    noise_new = np.random.default_rng(78).uniform(0.01, 0.5, n_b)
    c = pf.NOISE + pf.SIGMA
    d = np.r_[np.full(m0, c), noise_new + pf.SIGMA]
    ref = dense_reference(host.values, host.vectors[rows], d, Y, Uu, K)
    h0 = api.Predictor.regression(model, pair, Y[:m0], idx0, K, (pf.T, pf.NOISE), pf.SIGMA)
    h1 = h0.update(X[idxb], Y[m0:], noise=noise_new)
    got = judge(h1, Xu, ref, m0 + n_b, c, f"{shape} {kernel} per-row noise, updated")
    # the fresh "different" create: its mean is the comparator; its variance is built at noise[0] by design and is not
    fresh = api.Predictor.regression(model, pair, Y, rows, K, (pf.T, *np.r_[np.full(m0, pf.NOISE), noise_new]), pf.SIGMA, noisepar="different")
    fm = fresh.apply(Xu, var=False)["mean"]
    b_mean = rc.atol_mean(ref[0].astype(np.float64))
    r_fresh = float(np.abs(fm.astype(LD) - ref[0]).max()) / b_mean
    r_pair = float(np.abs(fm - got["mean"]).max()) / (2 * b_mean)
    print(f"{shape} {kernel} per-row noise: fresh mean |d| / bound {r_fresh:.3e}, updated against fresh / (2 bound) {r_pair:.3e}")
    assert r_fresh <= 1.0 and r_pair <= 1.0
    # the handle the update returned is consistent: it can be updated again, with one noise for all rows
    h2 = h1.update(X[idx0[:3]], Y[:3], noise=0.2)
    assert h2.kind == "regression"
    for h in (h0, h1, h2, fresh):
        h.free()


@pytest.mark.parametrize("shape,kernel", [("A", "se"), ("As", "lae")])
def test_chained_updates(shape, kernel):
    K = pf.SHAPES[shape][4]
    X = pf.case(shape)[0]
    model, pair, host = pf.fitted(shape, kernel)
    Xu, Uu = unseen(shape, kernel)
    m0, na, nb, q = 12, 30, 41, 3
    idx0, idxb, Y = labelled(shape, m0, na + nb, q, seed=55)
    rows = np.r_[idx0, idxb]
    c = pf.NOISE + pf.SIGMA
    m = m0 + na + nb
    ref = dense_reference(host.values, host.vectors[rows], np.full(m, c), Y, Uu, K)
    h0 = api.Predictor.regression(model, pair, Y[:m0], idx0, K, (pf.T, pf.NOISE), pf.SIGMA)
    ha = h0.update(X[idxb[:na]], Y[m0:m0 + na])
    hab = ha.update(X[idxb[na:]], Y[m0 + na:])
    both = h0.update(X[idxb], Y[m0:])
    fresh = api.Predictor.regression(model, pair, Y, rows, K, (pf.T, pf.NOISE), pf.SIGMA)
    got = [judge(h, Xu, ref, m, c, f"{shape} {kernel} {name}") for h, name in ((hab, "A then B"), (both, "A u B"), (fresh, "fresh"))]
    b_mean = rc.atol_mean(ref[0].astype(np.float64))
    b_var = rc.atol_var(dict(var=ref[1].astype(np.float64) + c, prior=ref[3], m=m, c=c))
    for a in range(3):
        for b in range(a + 1, 3):
            assert np.abs(got[a]["mean"] - got[b]["mean"]).max() <= 2 * b_mean and np.abs(got[a]["var"] - got[b]["var"]).max() <= 2 * b_var
    for h in (h0, ha, hab, both, fresh):
        h.free()


@pytest.mark.parametrize("shape,kernel", [("A", "lae"), ("As", "lae")])
def test_invariants(shape, kernel):
    K = pf.SHAPES[shape][4]
    X = pf.case(shape)[0]
    model, pair, host = pf.fitted(shape, kernel)
    Xu, _ = unseen(shape, kernel)
    m0, n_b, q = 60, 300, 3
    idx0, idxb, Y = labelled(shape, m0, n_b, q, seed=91)
    h0 = api.Predictor.regression(model, pair, Y[:m0], idx0, K, (pf.T, pf.NOISE), pf.SIGMA)
    before = h0.to_host()
    old = h0.apply(Xu)
    Z = h0.features(Xu)
    h1 = h0.update(X[idxb], Y[m0:])
    after = h0.to_host()
    np.testing.assert_array_equal(after["P"], before["P"]); np.testing.assert_array_equal(after["cg"], before["cg"])
    h0.free()                                                                    # the new handle borrows the model, not h0
    new = h1.apply(Xu)
    t = h1.to_host()
    np.testing.assert_array_equal(t["cg"], before["cg"])
    assert (t["P"][:, K + q:] == 0.0).all()                                      # the padding stays zero
    assert (new["var"][:, 0] >= t["cg"][0]).all()                                # bit for bit: cg plus a sum of squares
    slack = (K + 8) * 2.0 ** -53 * (Z * Z).sum(1)
    ratio = float(((new["var"][:, 0].astype(LD) - old["var"][:, 0].astype(LD)) / slack.astype(LD)).max())
    print(f"{shape} {kernel}: largest (var' - var) / ((K + 8) u sum z^2) = {ratio:.3e}")
    assert ratio <= 1.0
    assert (new["var"][:, 0] < old["var"][:, 0]).mean() > 0.9                    # and it did learn something
    Z1 = h1.features(Xu[:NCOV])
    C1 = h1.covariance(Xu[:NCOV])
    assert Z1.shape == (NCOV, K) and np.isfinite(Z1).all()
    np.testing.assert_array_equal(C1, C1.T)
    dr = h1.draws(4, seed=5)
    f = dr.apply(Xu[:NCOV])
    assert f.shape == (NCOV, 1, q, 4) and np.isfinite(f).all()
    dr.free(); h1.free()


def _dev_update(h, model, Xb, Yb, noise=None):
    """flgp_dev_predictor_update on padded device buffers"""
    import torch
    L = _lib.lib()
    n, d = Xb.shape
    q = Yb.shape[1]
    ldx, ldy = n + 3, n + 5
    dX = torch.full((d, ldx), float("nan"), dtype=torch.float64, device=pf.DEV); dX[:, :n] = torch.from_numpy(np.ascontiguousarray(Xb.T)).to(pf.DEV)
    dY = torch.full((q, ldy), float("nan"), dtype=torch.float64, device=pf.DEV); dY[:, :n] = torch.from_numpy(np.ascontiguousarray(Yb.T)).to(pf.DEV)
    dn = None if noise is None else torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float64)).to(pf.DEV)
    out = ctypes.c_void_p()
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(L.flgp_dev_predictor_update(st, h._h, dX.data_ptr(), n, ldx, dY.data_ptr(), ldy, None if dn is None else dn.data_ptr(),
                                           0 if dn is None else dn.numel(), ctypes.byref(out)))
    torch.cuda.synchronize()
    return api.Predictor(out, model)


def test_the_same_bits_whatever_the_block_and_the_entry():
    shape, kernel = "A", "lae"
    K = pf.SHAPES[shape][4]
    X = pf.case(shape)[0]
    model, pair, host = pf.fitted(shape, kernel)
    m0, n_b, q = 60, 2500, 3                                                      # ten chunks of the Gram kernel
    idx0, idxb, Y = labelled(shape, m0, n_b, q, seed=13)
    noise_new = np.random.default_rng(14).uniform(0.01, 0.5, n_b)
    h0 = api.Predictor.regression(model, pair, Y[:m0], idx0, K, (pf.T, pf.NOISE), pf.SIGMA)
    L = _lib.lib()
    want = h0.update(X[idxb], Y[m0:], noise=noise_new)
    P = want.to_host()["P"]
    assert np.isfinite(P).all()
    L.flgp_set_tuning(b"model_extend_block", 256)
    try:
        small = h0.update(X[idxb], Y[m0:], noise=noise_new)
        dev_small = _dev_update(h0, model, X[idxb], Y[m0:], noise_new)
    finally:
        L.flgp_set_tuning(b"model_extend_block", 1 << 20)
    dev = _dev_update(h0, model, X[idxb], Y[m0:], noise_new)
    for h in (small, dev_small, dev):
        np.testing.assert_array_equal(h.to_host()["P"], P)
        h.free()
    # noise = None is the create's noise[0], and so is that value given once or per row
    a = h0.update(X[idxb[:40]], Y[m0:m0 + 40]).to_host()["P"]
    for nz in (pf.NOISE, np.full(40, pf.NOISE)):
        np.testing.assert_array_equal(h0.update(X[idxb[:40]], Y[m0:m0 + 40], noise=nz).to_host()["P"], a)
    np.testing.assert_array_equal(_dev_update(h0, model, X[idxb[:40]], Y[m0:m0 + 40]).to_host()["P"], a)
    want.free(); h0.free()


def test_refusals_that_need_live_handles():
    shape = "A"
    K = pf.SHAPES[shape][4]
    X = pf.case(shape)[0]
    model, pair, host = pf.fitted(shape, "lae")
    m0, n_b, q = 60, 9, 1
    idx0, idxb, Y = labelled(shape, m0, n_b, q, seed=3)
    Xb, Yb = X[idxb], Y[m0:]
    ybin = (Y[:m0, 0] > 0).astype(float)
    reg = api.Predictor.regression(model, pair, Y[:m0], idx0, K, (pf.T, pf.NOISE), pf.SIGMA)
    logit = api.Predictor.logit(model, pair, idx0, K, [1.5], ybin)
    pg = api.Predictor.pg(model, pair, idx0, K, [1.5], ybin, pf.SIGMA, seed=4, N_sample=3)
    draws = reg.draws(2, seed=1)
    diff = api.Predictor.regression(model, pair, Y[:m0], idx0, K, (pf.T, *np.full(m0, pf.NOISE)), pf.SIGMA, noisepar="different")
    Xn, Un, _ = pf.ny_cloud()
    grid, pairs = pf.ny_fitted()
    i0n, Yn = pf.training(Xn, 20, 1, seed=8)
    ny = api.Predictor.nystrom_regression(grid, 0, pairs[0], Yn, i0n, pf.NY[3], (pf.T, pf.NOISE), pf.SIGMA)
    for h, text in ((logit, "a logit handle cannot be updated \\(a Laplace posterior is not closed under conditioning\\)"),
                    (pg, "a Polya-Gamma handle cannot be updated"), (draws, "a draws handle cannot be updated"),
                    (diff, "the handle was created with per-row noise")):
        with pytest.raises(api.FlgpError, match="predictor_update: " + text):
            h.update(Xb, Yb if h.q == 1 else np.zeros((n_b, h.q)))
    with pytest.raises(api.FlgpError, match="predictor_update: a Nystrom handle cannot be updated"):
        ny.update(Xn[:n_b], Yb)
    # a bad noise length, at the library
    out = ctypes.c_void_p(1)
    xb = np.asfortranarray(Xb); nz = np.full(4, 0.1)
    rc_ = _lib.lib().flgp_predictor_update(reg._h, xb.ctypes.data, n_b, Yb.ctypes.data, nz.ctypes.data, 4, ctypes.byref(out))
    assert rc_ == -1 and out.value is None and "n_noise=4 must be 0 with a NULL noise, 1 or n_b=9" in _lib.lib().flgp_last_error().decode()
    # values: Y, the noise, noise + sigma, X
    bad = Yb.copy(); bad[4, 0] = np.inf
    with pytest.raises(api.FlgpError, match="predictor_update: the responses Y"):
        reg.update(Xb, bad)
    with pytest.raises(api.FlgpError, match="predictor_update: noise\\[0\\] must be finite"):
        reg.update(Xb, Yb, noise=np.nan)
    nzb = np.full(n_b, 0.1); nzb[5] = -pf.SIGMA
    with pytest.raises(api.FlgpError, match="predictor_update: noise\\[5\\] \\+ sigma must be positive"):
        reg.update(Xb, Yb, noise=nzb)
    good = reg.apply(X[:70])
    xbad = np.array(Xb, order="F"); xbad[2, 1] = np.nan
    with pytest.raises(api.FlgpError, match="points"):
        reg.update(xbad, Yb)
    after = reg.apply(X[:70])
    for key in ("mean", "var"):
        np.testing.assert_array_equal(after[key], good[key])
    ok = reg.update(Xb, Yb)
    assert ok.kind == "regression"
    for h in (ok, reg, logit, pg, draws, diff, ny):
        h.free()
