"""GPU (-m gpu): the Polya-Gamma predictor on a fitted spectrum model (include/flgp_hip.h) on the fits of
tests/test_gpu_predictor.py ("A": n 3000, d 3, s 200, r 5, K 20 with the kernels "lae" and "se"; "wide": d 70), made once per
module.  N_sample = 8; m = 60 > K and m = 12 <= K, so both chain routes run; B = 3 chains, the third a duplicate of the first.

* fit rows: predict(X[idx1]) against test_pgbinary_batch(.., sigma_nv=0) on the same pair;
* new rows: 300 rows of another draw against model.extend(.., resident, head = the training rows) + the batch entry on the
  stacked pair.
  Tolerance of both: the project's form for a reassociated mean, atol_mean = 1e-9 F of tests/regression_posterior_cases.py
  with F = max |log(pi_ref / (1 - pi_ref))| from the batch entry's output (asserted below 20, so that the scale does not come
  from the code under test); the logistic is 1/4-Lipschitz, so |pi - pi_ref| <= tol_pi = 0.25 atol_mean + 8 * 2^-53.  |d| is
  printed beside the bound.  y is compared where |pi_ref - 0.5| > tol_pi and label where the gap between the largest pi_ref
  and the largest of the chains that are not its duplicates exceeds 2 tol_pi (a duplicate has the same bits on both sides);
  on the chosen seeds no row falls outside these sets: asserted on the batch entry's output;
* omega and f of the chains are the batch entry's, bit for bit;
* pg_for_classes against predict_logit_mult_gp_batch under the same condition;
* bits: 513 rows as one call, in blocks of 256 and one at a time; the host and the device entry; column b of P and of every
  output for B = 1, B = 3 in two orders and max_parallel 0, 1, 2;
* to_host(): P against the restatement Bq u (tests/np_predictor_pg.py), u from tests/np_pg.py's collapsed weights at
  omega_out, to 1e-9 max|P| (np_pg's own tolerance);
* the refusals that need live handles."""
import functools

import numpy as np
import pytest

import np_predictor as npp
import np_predictor_pg as npg
from conftest import make_case
from flgp_amd import _lib, api, synth
from predictor_pg_checks import bounds, compare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = {"A": (3000, 3, 200, 5, 20), "wide": (600, 70, 64, 5, 10)}
EPSILON = {"A": 0.7, "wide": 6.0}
SIGMA, NS = 1e-2, 8
TS = np.array([1.5, 4.0, 1.5])
TS_OF = {"A": TS, "wide": 4.0 * TS}          # "wide": a tighter prior, for the same reason as its labels (problem())
COL = np.array([0, 1, 0], dtype=np.int32)
SEEDS = [901, 902, 901]                      # chain 2 is chain 0 again


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()


@functools.lru_cache(maxsize=None)
def case(shape):
    n, d, s, r, K = SHAPES[shape]
    X, U0, U = make_case(n, d, s, r, seed=n + d)
    for a in (X, U0, U):
        a.setflags(write=False)
    return X, U0, U


@functools.lru_cache(maxsize=None)
def fitted(shape, kernel="lae"):
    """(model, pair, the pair on the host): one fit per configuration, shared and left unchanged"""
    n, d, s, r, K = SHAPES[shape]
    X, U0, U = case(shape)
    model, pair = api.heat_kernel_spectrum_model(X, X[:0], s, r, K, models={"kernel": kernel, "gl": "cluster-normalized", "root": True},
                                                 epsilon=EPSILON[shape], U=U)
    host = pair.to_host()
    host.values.setflags(write=False); host.vectors.setflags(write=False)
    return model, pair, host


def problem(shape, m, seed=21):
    """two label columns, a threshold on a coordinate each.  On "wide" the thresholded coordinate carries noise of its own
    size: clean labels drive the latent of these chains past 20 there, and the tolerance below is stated for |f| < 20"""
    X = case(shape)[0]
    rng = np.random.default_rng(seed)
    idx0 = rng.permutation(SHAPES[shape][0])[:m].astype(np.int32)
    Z = X[idx0, :2] + (X[idx0, :2].std(axis=0) * rng.normal(size=(m, 2)) if shape == "wide" else 0.0)
    Y = np.asfortranarray((Z > np.median(Z, axis=0)).astype(float))
    return idx0, Y


def make(model, pair, idx0, K, Y, **kw):
    kw = dict(dict(col=COL, seeds=SEEDS, N_sample=NS), **kw)
    return api.Predictor.pg(model, pair, idx0, K, kw.pop("ts", TS), Y, SIGMA, **kw)


def make_of(shape, model, pair, idx0, K, Y, **kw):
    return make(model, pair, idx0, K, Y, ts=TS_OF[shape], **kw)


# ------------------------------------------------------------------------------------------------------- 1. fit rows
@pytest.mark.parametrize("shape,kernel,m", [("A", "lae", 60), ("A", "lae", 12), ("A", "se", 60), ("wide", "lae", 60)])
def test_fit_rows_against_the_batch_entry(shape, kernel, m):
    n, d, s, r, K = SHAPES[shape]
    X = case(shape)[0]
    model, pair, host = fitted(shape, kernel)
    idx0, Y = problem(shape, m)
    rows = np.random.default_rng(5).permutation(n)[:257].astype(np.int32)
    ref = pair.test_pgbinary_batch(idx0, rows, K, TS_OF[shape], Y, SIGMA, 0.0, col=COL, seeds=SEEDS, N_sample=NS, output_pi=True,
                                   return_state=True, return_argmax=True)
    pred, state = make_of(shape, model, pair, idx0, K, Y, return_state=True)
    assert pred.dims == {"d": d, "s": s, "r": r, "K": K, "groups": 1, "q": 3, "kind": "pg", "ldp": 16}
    np.testing.assert_array_equal(state["omega"], ref["omega"])
    np.testing.assert_array_equal(state["f"], ref["f"])
    got = pred.predict(X[rows], latent=True)
    compare(got, ref, f"fit rows {shape} {kernel} m={m}")
    np.testing.assert_array_equal(got["f"][:, 0], got["f"][:, 2])                      # the duplicated chain
    host_out = pred.to_host()
    assert (host_out["P"][:, 3:] == 0.0).all() and (host_out["cg"] == 0.0).all()
    # the existing apply gives the latent and has no variance to give
    np.testing.assert_array_equal(pred.apply(X[rows], var=False)["mean"], got["f"])
    with pytest.raises(api.FlgpError, match="predictor_apply: a Polya-Gamma handle has no variance"):
        pred.apply(X[rows])
    pred.free(); pred.free()
    with pytest.raises(ValueError, match="freed"):
        pred.predict(X[rows])


# ------------------------------------------------------------------------------------------------------- 2. new rows
@pytest.mark.parametrize("shape,kernel,m", [("A", "lae", 60), ("A", "se", 60), ("A", "se", 12), ("wide", "lae", 60)])
def test_new_rows_against_the_extension_route(shape, kernel, m):
    n, d, s, r, K = SHAPES[shape]
    model, pair, host = fitted(shape, kernel)
    idx0, Y = problem(shape, m)
    X2 = synth.gaussian_mixture(300, d, components=5, seed=n + d + 1000)               # another draw: none of the fit rows
    both = model.extend(X2, resident=True, head=pair, head_rows=idx0)
    i0, i1 = np.arange(m, dtype=np.int32), m + np.arange(300, dtype=np.int32)
    ref = both.test_pgbinary_batch(i0, i1, K, TS_OF[shape], Y, SIGMA, 0.0, col=COL, seeds=SEEDS, N_sample=NS, output_pi=True,
                                   return_state=True, return_argmax=True)
    pred, state = make_of(shape, model, pair, idx0, K, Y, return_state=True)
    np.testing.assert_array_equal(state["omega"], ref["omega"])
    np.testing.assert_array_equal(state["f"], ref["f"])
    compare(pred.predict(X2), ref, f"new rows {shape} {kernel} m={m}")
    both.free(); pred.free()


# ----------------------------------------------------------------------------------------------------- 3. multiclass
@pytest.mark.parametrize("m", [60, 12])
def test_classes_against_the_one_vs_rest_batch(m):
    shape = "A"
    n, d, s, r, K = SHAPES[shape]
    X = case(shape)[0]
    model, pair, host = fitted(shape)
    idx0 = np.random.default_rng(31).permutation(n)[:m].astype(np.int32)
    q = np.quantile(X[idx0, 0], [1.0 / 3.0, 2.0 / 3.0])
    labels = np.digitize(X[idx0, 0], q).astype(float)                                  # three classes along the first coordinate
    ts = np.array([1.5, 2.5, 4.0])
    rows = np.random.default_rng(6).permutation(n)[:257].astype(np.int32)
    lab_ref, probs = pair.predict_logit_mult_gp_batch(idx0, rows, K, ts, labels, SIGMA, N_sample=NS, seed=77, output_probs=True)
    tol = bounds(probs)
    pred = api.Predictor.pg_for_classes(model, pair, idx0, K, ts, labels, SIGMA, N_sample=NS, seed=77)
    got = pred.predict(X[rows])
    d_ = np.abs(got["pi"] - probs).max()
    print(f"classes m={m}: |pi - probs| {d_:.3e} bound {tol:.3e} ratio {d_ / tol:.3e}")
    assert d_ <= tol
    np.testing.assert_array_equal(got["label"], lab_ref)
    assert len(set(lab_ref.tolist())) > 1
    pred.free()


# ------------------------------------------------------------------------------------------------------------- 4. bits
def test_bits_do_not_depend_on_the_call():
    import torch
    shape = "A"
    n, d, s, r, K = SHAPES[shape]
    model, pair, host = fitted(shape)
    idx0, Y = problem(shape, 60)
    pred = make(model, pair, idx0, K, Y)
    X2 = np.asfortranarray(synth.gaussian_mixture(513, d, components=5, seed=99))
    L = _lib.lib()
    want = pred.predict(X2, latent=True)
    keys = ("f", "pi", "y", "label")
    L.flgp_set_tuning(b"model_extend_block", 256)
    try:
        small = pred.predict(X2, latent=True)
        # the device-pointer entry on padded buffers
        n_new, ldx, ld = 513, 516, {"f": 518, "pi": 515, "y": 514}
        dX = torch.full((d, ldx), float("nan"), dtype=torch.float64, device=DEV)
        dX[:, :n_new] = torch.from_numpy(np.ascontiguousarray(X2.T)).to(DEV)
        buf = {k: torch.full((4, ld[k]), float("nan"), dtype=torch.float64, device=DEV) for k in ld}
        lab = torch.full((n_new + 3,), float("nan"), dtype=torch.float64, device=DEV)
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(L.flgp_dev_predictor_pg_apply(st, pred._h, dX.data_ptr(), n_new, ldx, buf["f"].data_ptr(), ld["f"],
                                                 buf["pi"].data_ptr(), ld["pi"], buf["y"].data_ptr(), ld["y"], lab.data_ptr()))
        torch.cuda.synchronize()
    finally:
        L.flgp_set_tuning(b"model_extend_block", 1 << 20)
    for k in keys:
        np.testing.assert_array_equal(small[k], want[k], err_msg=k)
    for k in ld:
        a = buf[k].cpu().numpy()
        np.testing.assert_array_equal(a[:3, :n_new].T, want[k], err_msg=k)
        assert np.isnan(a[3]).all() and np.isnan(a[:, n_new:]).all()
    a = lab.cpu().numpy()
    np.testing.assert_array_equal(a[:n_new], want["label"]); assert np.isnan(a[n_new:]).all()
    for i in (0, 255, 256, 300, 512):
        one = pred.predict(X2[i:i + 1], latent=True)
        for k in keys:
            np.testing.assert_array_equal(one[k][0], want[k][i], err_msg=f"{k} row {i}")
    np.testing.assert_array_equal(pred.predict(X2)["pi"], want["pi"])                  # without the latent


@pytest.mark.parametrize("m", [60, 12])
def test_a_column_depends_on_its_chain_alone(m):
    shape = "A"
    n, d, s, r, K = SHAPES[shape]
    model, pair, host = fitted(shape)
    idx0, Y = problem(shape, m)
    X2 = np.asfortranarray(synth.gaussian_mixture(70, d, components=5, seed=98))
    pred, state = make(model, pair, idx0, K, Y, return_state=True)
    P = pred.to_host()["P"]
    want = pred.predict(X2, latent=True)
    for mp in (1, 2):
        other, st2 = make(model, pair, idx0, K, Y, max_parallel=mp, return_state=True)
        np.testing.assert_array_equal(other.to_host()["P"], P)
        for k in ("omega", "f"):
            np.testing.assert_array_equal(st2[k], state[k])
        other.free()
    # the three chains in another order
    order = [1, 2, 0]
    swapped = make(model, pair, idx0, K, Y, ts=TS[order], col=COL[order], seeds=[SEEDS[b] for b in order])
    assert swapped.q == 3
    np.testing.assert_array_equal(swapped.to_host()["P"][:, :3], P[:, order])
    got = swapped.predict(X2, latent=True)
    for k in ("f", "pi", "y"):
        np.testing.assert_array_equal(got[k], want[k][:, order], err_msg=k)
    swapped.free()
    for b in range(3):
        alone = make(model, pair, idx0, K, Y, ts=TS[b:b + 1], col=COL[b:b + 1], seeds=SEEDS[b:b + 1])
        assert (alone.q, alone.ldp) == (1, 16)
        np.testing.assert_array_equal(alone.to_host()["P"][:, 0], P[:, b])
        got = alone.predict(X2, latent=True)
        for k in ("f", "pi", "y"):
            np.testing.assert_array_equal(got[k][:, 0], want[k][:, b], err_msg=f"{k} chain {b}")
        assert (got["label"] == 0.0).all()
        alone.free()
    pred.free()


# ---------------------------------------------------------------------------------------------------- 5. to_host
@pytest.mark.parametrize("m", [60, 12])
def test_P_is_the_restatement(m):
    shape = "A"
    n, d, s, r, K = SHAPES[shape]
    model, pair, host = fitted(shape)
    idx0, Y = problem(shape, m)
    pred, state = make(model, pair, idx0, K, Y, return_state=True)
    P = pred.to_host()["P"]
    h = model.to_host()
    Bq = npp.anchor_side(h["V"], h["eig"], n, K)
    V1 = host.vectors[idx0, :K]
    U = np.stack([npg.chain_u(V1, host.values, K, TS[b], SIGMA, state["omega"][:, b], Y[:, COL[b]]) for b in range(3)], axis=1)
    Pn = npg.fold(Bq, U)
    dP = np.abs(P[:, :3] - Pn).max()
    print(f"P against the restatement m={m}: |d| {dP:.3e}, 1e-9 max|P| = {1e-9 * np.abs(Pn).max():.3e}")
    assert np.abs(Pn).max() > 0.0 and dP <= 1e-9 * np.abs(Pn).max()
    pred.free()


# ------------------------------------------------------------------------------------------------- 6. live refusals
def test_refusals_that_need_live_handles():
    shape = "A"
    n, d, s, r, K = SHAPES[shape]
    X = case(shape)[0]
    model, pair, host = fitted(shape)
    idx0, Y = problem(shape, 60)
    other_model, other_pair, _ = fitted(shape, "se")
    with pytest.raises(api.FlgpError, match="predictor_pg: the pair's values are not the model's"):
        make(model, other_pair, idx0, K, Y)
    narrow = api.ResidentEigenPair.from_host(api.EigenPair(host.values[:13].copy(), np.asfortranarray(host.vectors[:, :13])))
    with pytest.raises(api.FlgpError, match="predictor_pg: the pair has K = 13, the model K = 20"):
        make(model, narrow, idx0, 13, Y)
    with pytest.raises(api.FlgpError, match=r"predictor_pg: need 1 <= K <= 13 \(K=20\)"):
        make(model, narrow, idx0, 20, Y)                                               # the chains' refusal comes first
    narrow.free()
    with pytest.raises(api.FlgpError, match="predictor_pg: idx0"):
        make(model, pair, np.r_[idx0[:-1], n].astype(np.int32), K, Y)
    # the C entries on a handle of another kind
    reg = api.Predictor.regression(model, pair, Y[:, :1], idx0, K, (2.0, 0.1), 1e-3)
    L = _lib.lib()
    Xf = np.asfortranarray(X[:5]); out = np.zeros(5)
    assert L.flgp_predictor_pg_apply(reg._h, Xf.ctypes.data, 5, None, None, None, out.ctypes.data) == -1
    assert L.flgp_last_error().decode() == "predictor_pg_apply: the handle is not a Polya-Gamma one (kind 0)"
    with pytest.raises(api.FlgpError, match="not a Polya-Gamma one"):
        reg.predict(X[:5])
    reg.free()
    # a NaN in X is the input check's refusal, and the handle stays usable
    pred = make(model, pair, idx0, K, Y)
    good = pred.predict(X[:70], latent=True)
    bad = np.array(X[:70], order="F"); bad[17, 1] = np.nan
    with pytest.raises(api.FlgpError, match="points"):
        pred.predict(bad)
    after = pred.predict(X[:70], latent=True)
    for k in good:
        np.testing.assert_array_equal(after[k], good[k])
    with pytest.raises(api.FlgpError, match="a Polya-Gamma handle has no variance"):
        pred.apply(X[:70], var=True)
    with pytest.raises(ValueError, match="columns"):
        pred.predict(np.zeros((4, d + 1)))
    pred.free()
