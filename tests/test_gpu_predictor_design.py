"""GPU (-m gpu): flgp_predictor_design / flgp_dev_predictor_design (include/flgp_hip.h) on the fits of
tests/predictor_joint_fits.py: "A" (K = 20) and "As" (K = 200), "lae" and "se", a regression handle on 60 labelled rows at
T, NOISE, SIGMA, a pool of 1000 unseen rows, B in {1, 7, 40}.

* The host and the device entry, and model_extend_block in {256, 1 << 20}, give the same bits; so does the restatement
  (tests/np_predictor_design.py) on the model's own ELL rows and the handle's P; B = 1 and 7 are prefixes of B = 40.
* Optimal at every step, none left out: Z = features(pool) is taken as data; for every t the long-double conditional variance
  given the device's own picks[:t] is computed, and the picked row's must be at least the largest over the untaken rows minus
  twice the bound of f-25 (np_predictor_design.bound: operation counts times 2^-53 times sums of absolute terms).
* score against that reference at t = B within the bound; the largest ratio is printed (recorded in DESIGN f-25).
* score + cg against update(h, X[picks], Y).apply(var) within twice f-24's atol_var: both approximate one long-double value.
* The live refusals 4 to 9 with their sentences; h serves the same bits afterwards.  Predictor.design round-trips."""
import ctypes
import functools

import numpy as np
import pytest

import np_predictor_design as nd
import predictor_joint_fits as pf
import regression_posterior_cases as rc
from flgp_amd import _lib, api

pytestmark = pytest.mark.gpu
LD = pf.LD
POOL, M0, BMAX = 1000, 60, 40
FITS = [("A", "lae"), ("A", "se"), ("As", "lae"), ("As", "se")]


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()


@functools.lru_cache(maxsize=None)
def pool(shape):
    X = pf.new_rows(shape, POOL, seed=2500)
    X.setflags(write=False)
    return X


def handle(shape, kernel, q=1):
    K = pf.SHAPES[shape][4]
    model, pair, host = pf.fitted(shape, kernel)
    idx0, Y = pf.training(pf.case(shape)[0], M0, q, seed=31)
    return api.Predictor.regression(model, pair, Y, idx0, K, (pf.T, pf.NOISE), pf.SIGMA)


def _dev_design(h, X, B, noise=None):
    """flgp_dev_predictor_design on padded device buffers"""
    import torch
    L = _lib.lib()
    n, d = X.shape
    ldx = n + 3
    dX = torch.full((d, ldx), float("nan"), dtype=torch.float64, device=pf.DEV); dX[:, :n] = torch.from_numpy(np.array(X.T, order="C")).to(pf.DEV)
    picks = torch.full((B + 2,), -7, dtype=torch.int32, device=pf.DEV)
    gain = torch.full((B + 2,), float("nan"), dtype=torch.float64, device=pf.DEV)
    score = torch.full((n + 2,), float("nan"), dtype=torch.float64, device=pf.DEV)
    nz = None if noise is None else np.array([noise], dtype=np.float64)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(L.flgp_dev_predictor_design(st, h._h, dX.data_ptr(), n, ldx, B, None if nz is None else nz.ctypes.data, picks.data_ptr(),
                                           gain.data_ptr(), score.data_ptr()))
    torch.cuda.synchronize()
    assert (picks[B:] == -7).all().item() and torch.isnan(gain[B:]).all().item() and torch.isnan(score[n:]).all().item()
    return {"picks": picks[:B].cpu().numpy(), "gain": gain[:B].cpu().numpy(), "var": score[:n].cpu().numpy()}


def _same(a, b, label):
    for key in ("picks", "gain", "var"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=f"{label}: {key}")


@pytest.mark.parametrize("shape,kernel", [("A", "lae"), ("As", "se")])
def test_the_same_bits_whatever_the_block_the_entry_and_the_restatement(shape, kernel):
    K = pf.SHAPES[shape][4]
    X = pool(shape)
    h = handle(shape, kernel)
    L = _lib.lib()
    want = h.design(X, BMAX)
    assert want["picks"].dtype == np.int32 and want["picks"].shape == (BMAX,) and want["gain"].shape == (BMAX,) and want["var"].shape == (POOL,)
    assert len(set(want["picks"].tolist())) == BMAX and (np.diff(want["gain"]) <= 0).all()
    L.flgp_set_tuning(b"model_extend_block", 256)
    try:
        _same(h.design(X, BMAX), want, "host, blocks of 256")
        _same(_dev_design(h, X, BMAX), want, "device, blocks of 256")
    finally:
        L.flgp_set_tuning(b"model_extend_block", 1 << 20)
    _same(_dev_design(h, X, BMAX), want, "device, one block")
    _same(h.design(X, BMAX, noise=pf.NOISE), want, "the create's noise given")
    for B in (1, 7):
        got = h.design(X, B)
        np.testing.assert_array_equal(got["picks"], want["picks"][:B]); np.testing.assert_array_equal(got["gain"], want["gain"][:B])
    idx, val = pf.model_ell_rows(shape, kernel, X)
    picks, gain, score = nd.design(idx, val, h.to_host()["P"], K, pf.NOISE + pf.SIGMA, BMAX)
    _same(dict(picks=picks, gain=gain, var=score), want, "the restatement")
    h.free()


@pytest.mark.parametrize("shape,kernel", FITS)
def test_optimal_at_every_step_and_the_scores_within_the_bound(shape, kernel):
    n_fit, dim, s, r, K = pf.SHAPES[shape]
    X = pool(shape)
    h = handle(shape, kernel)
    d = pf.NOISE + pf.SIGMA
    got = h.design(X, BMAX)
    picks = got["picks"]
    Z = h.features(X)
    idx, val = pf.model_ell_rows(shape, kernel, X)
    absZ = nd.npd.cols(idx, np.abs(val), np.abs(h.to_host()["P"]), 0, K)
    Zl = Z.astype(LD)
    Kx = Zl[picks] @ Zl.T                                                          # once: step t uses its first t rows
    for t in range(BMAX + 1):
        ref, alpha = nd.cond_var(Z, picks[:t], d, Kx=Kx[:t])
        bnd = nd.bound(absZ, picks[:t], alpha, d, K, r)
        if t < BMAX:
            free = np.ones(POOL, dtype=bool); free[picks[:t]] = False
            j = picks[t]
            assert free[j], t
            assert ref[j] >= (ref[free] - bnd[free]).max() - bnd[j], f"{shape} {kernel}: step {t} is not optimal"
            assert abs(LD(got["gain"][t]) - ref[j]) <= bnd[j], t
    ratio = float((np.abs(got["var"].astype(LD) - ref) / bnd).max())
    print(f"{shape} {kernel}: |score - score_ld| / bound at B = {BMAX}: {ratio:.3e} (largest bound {float(bnd.max()):.2e}, "
          f"largest score {got['var'].max():.3e})")
    assert ratio <= 1.0
    h.free()


@pytest.mark.parametrize("noise", [None, 0.3])
@pytest.mark.parametrize("shape,kernel", [("A", "se"), ("As", "lae")])
def test_the_scores_are_the_updated_handles_variance(shape, kernel, noise):
    K = pf.SHAPES[shape][4]
    X = pool(shape)
    model, pair, host = pf.fitted(shape, kernel)
    q = 3
    h = handle(shape, kernel, q)
    got = h.design(X, BMAX, noise=noise)
    picks = got["picks"]
    Y = np.asfortranarray(np.random.default_rng(5).normal(size=(BMAX, q)))         # whatever Y is
    h1 = h.update(X[picks], Y, noise=noise)
    var = h1.apply(X)["var"][:, 0]
    cg = h.to_host()["cg"][0]
    c = pf.NOISE + pf.SIGMA
    Uu = model.extend(X).vectors
    lam = np.exp(-pf.T * (1 - np.asarray(host.values[:K])))
    prior = float(((Uu[:, :K] ** 2) * lam).sum(1).max())
    b_var = rc.atol_var(dict(var=var, prior=prior, m=M0 + BMAX, c=c))
    ratio = float(np.abs((got["var"] + cg) - var).max()) / (2 * b_var)
    print(f"{shape} {kernel} noise={noise}: |score + cg - update.apply(var)| / (2 atol_var) = {ratio:.3e}")
    assert ratio <= 1.0
    assert (got["var"][picks] < got["gain"]).all()                                 # a picked row did learn from its own label
    h1.free(); h.free()


def test_refusals_that_need_live_handles():
    shape = "A"
    K = pf.SHAPES[shape][4]
    X = pf.case(shape)[0]
    model, pair, host = pf.fitted(shape, "lae")
    idx0, Y = pf.training(X, M0, 1, seed=3)
    Xp = pool(shape)[:50]
    ybin = (Y[:, 0] > 0).astype(float)
    reg = api.Predictor.regression(model, pair, Y, idx0, K, (pf.T, pf.NOISE), pf.SIGMA)
    logit = api.Predictor.logit(model, pair, idx0, K, [1.5], ybin)
    pg = api.Predictor.pg(model, pair, idx0, K, [1.5], ybin, pf.SIGMA, seed=4, N_sample=3)
    draws = reg.draws(2, seed=1)
    diff = api.Predictor.regression(model, pair, Y, idx0, K, (pf.T, *np.full(M0, pf.NOISE)), pf.SIGMA, noisepar="different")
    Xn, Un, _ = pf.ny_cloud()
    grid, pairs = pf.ny_fitted()
    i0n, Yn = pf.training(Xn, 20, 1, seed=8)
    ny = api.Predictor.nystrom_regression(grid, 0, pairs[0], Yn, i0n, pf.NY[3], (pf.T, pf.NOISE), pf.SIGMA)
    good = reg.design(Xp, 5)
    served = reg.apply(X[:70])
    for hh, text in ((logit, "a logit handle has no design \\(the observation variance of a new label is not a constant\\)"),
                     (pg, "a Polya-Gamma handle has no design"), (draws, "a draws handle has no design"),
                     (diff, "the handle was created with per-row noise")):
        with pytest.raises(api.FlgpError, match="predictor_design: " + text):
            hh.design(Xp, 5)
    with pytest.raises(api.FlgpError, match="predictor_design: a Nystrom handle has no design"):
        ny.design(Xn[:50], 5)
    with pytest.raises(api.FlgpError, match="predictor_design: the noise must be finite"):
        reg.design(Xp, 5, noise=np.inf)
    with pytest.raises(api.FlgpError, match="predictor_design: the noise must be finite"):
        reg.design(Xp, 5, noise=np.nan)
    with pytest.raises(api.FlgpError, match="predictor_design: noise \\+ sigma must be positive"):
        reg.design(Xp, 5, noise=-pf.SIGMA)
    xbad = np.array(Xp, order="F"); xbad[2, 1] = np.nan
    with pytest.raises(api.FlgpError, match="points"):
        reg.design(xbad, 5)
    # the order: the kind is looked at before the noise and before X
    with pytest.raises(api.FlgpError, match="predictor_design: a logit handle has no design"):
        logit.design(xbad, 5, noise=np.nan)
    with pytest.raises(api.FlgpError, match="predictor_design: the noise must be finite"):
        reg.design(xbad, 5, noise=np.nan)
    again = reg.design(Xp, 5)
    for key in ("picks", "gain", "var"):
        np.testing.assert_array_equal(again[key], good[key])
    after = reg.apply(X[:70])
    for key in ("mean", "var"):
        np.testing.assert_array_equal(after[key], served[key])
    for hh in (reg, logit, pg, draws, diff, ny):
        hh.free()
