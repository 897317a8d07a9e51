"""GPU (-m gpu): the fitted spectrum model (include/flgp_hip.h).  The fit is the resident entry's bit for bit;
the extension of rows that were in the fit returns their rows of the fit's vectors bit for bit (every kernel x gl x root,
r up to 32, across the 256-row workgroups of the scaling kernel and the row blocks of the driver); the extension of new
rows is the numpy restatement of tests/np_spectrum_model.py bit for bit (LAE); flgp_dev_extend_scale alone is the three
passes it replaces; and the pair of `extend_resident` feeds the consumers as the fit's own pair does."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import np_sparse_stages as nps
import np_spectrum_model as npm
from conftest import make_case
from flgp_amd import _lib, api, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# n, d, s, r, K ("As", "B": K = s, the full decomposition)
SHAPES = {"A": (3000, 3, 200, 5, 20), "As": (3000, 3, 200, 5, 200), "B": (300, 3, 40, 4, 40), "wide": (600, 70, 64, 5, 10)}
COMBOS = list(itertools.product(("lae", "se"), npm.GLS, (False, True)))
# the SE bandwidth: not the default, so that the model has to carry it; at d = 70 squared distances are ~ 2 d
EPSILON = {"A": 0.7, "As": 0.7, "B": 0.7, "wide": 6.0}


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()


@functools.lru_cache(maxsize=None)
def case(shape, r=None):
    n, d, s, r0, K = SHAPES[shape]
    X, U0, U = make_case(n, d, s, r or r0, seed=n + d)
    for a in (X, U0, U):
        a.setflags(write=False)
    return X, U0, U


@functools.lru_cache(maxsize=None)
def fitted(shape, kernel, gl, root, r=None):
    """(model, pair, the pair on the host): one fit per configuration, shared by the tests and left unchanged"""
    n, d, s, r0, K = SHAPES[shape]
    X, U0, U = case(shape, r)
    model, pair = api.heat_kernel_spectrum_model(X, X[:0], s, r or r0, K, models={"kernel": kernel, "gl": gl, "root": root},
                                                 epsilon=EPSILON[shape], U=U)
    host = pair.to_host()
    host.values.setflags(write=False); host.vectors.setflags(write=False)
    return model, pair, host


def some_rows(n, count, seed=3):
    return np.random.default_rng(seed).permutation(n)[:count]


# ------------------------------------------------------------------------------------------------ 1. the fit is unchanged
@pytest.mark.parametrize("kernel,gl,root", COMBOS)
@pytest.mark.parametrize("shape", ["A", "B"])
def test_fit_is_the_resident_entry_bit_for_bit(shape, kernel, gl, root):
    n, d, s, r, K = SHAPES[shape]
    X, U0, U = case(shape)
    model, pair, host = fitted(shape, kernel, gl, root)
    ref = api.heat_kernel_spectrum_resident(X, X[:0], s, r, K, models={"kernel": kernel, "gl": gl, "root": root},
                                            epsilon=EPSILON[shape], U=U).to_host()
    np.testing.assert_array_equal(host.values, ref.values)
    np.testing.assert_array_equal(host.vectors, ref.vectors)
    assert (pair.n, pair.K) == (n, K)
    assert model.dims == {"n_fit": n, "d": d, "s": s, "r": r, "K": K, "kernel": kernel, "gl": gl, "root": root}
    np.testing.assert_array_equal(model.to_host()["values"], ref.values)


# -------------------------------------------------------------------------------------------------------- 2. frozen sums
@pytest.mark.parametrize("gl", npm.GLS)
@pytest.mark.parametrize("shape", ["A", "B"])
def test_frozen_column_sums_are_the_oracles(oracle, shape, gl):
    n, d, s, r, K = SHAPES[shape]
    X, U0, U = case(shape)
    got = fitted(shape, "lae", gl, False)[0].to_host()
    ei, z = oracle.lae(X, U0, r)
    sizes = np.ascontiguousarray(U[:, d])
    zn = oracle.graph_laplacian(ei, z, s, gl, sizes if gl == "cluster-normalized" else None)
    np.testing.assert_array_equal(got["colsum_gl"], np.zeros(s) if gl == "rw" else nps.colsum(ei, z, s))
    np.testing.assert_array_equal(got["colsum_spectrum"], nps.colsum(ei, zn, s))
    np.testing.assert_array_equal(got["sizes"], sizes if gl == "cluster-normalized" else np.zeros(s))
    assert got["V"].shape == (s, K) and got["eig"].shape == (K,)
    np.testing.assert_array_equal(got["values"], got["eig"])                     # root = False: sigma^2


# ------------------------------------------------------------------------------------- 3. fit rows come back exactly
@pytest.mark.parametrize("kernel,gl,root", COMBOS)
@pytest.mark.parametrize("shape", ["A", "B"])
def test_fit_rows_come_back_bit_for_bit(shape, kernel, gl, root):
    n = SHAPES[shape][0]
    X = case(shape)[0]
    model, pair, host = fitted(shape, kernel, gl, root)
    rows = some_rows(n, 277)                      # not n: a sqrt(n_new) in place of sqrt(n_fit) would show
    ep = model.extend(X[rows])
    np.testing.assert_array_equal(ep.vectors, host.vectors[rows])
    np.testing.assert_array_equal(ep.values, host.values)
    assert np.abs(ep.vectors).max() > 0.0


@pytest.mark.parametrize("kernel", ["lae", "se"])
@pytest.mark.parametrize("r", [1, 3, 10, 32])
def test_fit_rows_come_back_for_every_r(kernel, r):
    n = SHAPES["A"][0]
    X = case("A", r)[0]
    model, pair, host = fitted("A", kernel, "cluster-normalized", True, r)
    rows = some_rows(n, 301, seed=r)
    np.testing.assert_array_equal(model.extend(X[rows]).vectors, host.vectors[rows])


@pytest.mark.parametrize("kernel", ["lae", "se"])
def test_fit_rows_come_back_on_the_wide_route(kernel):
    """d = 70: the wide k-NN and the LDS LAE kernels"""
    n = SHAPES["wide"][0]
    X = case("wide")[0]
    model, pair, host = fitted("wide", kernel, "normalized", False)
    rows = some_rows(n, 259)
    np.testing.assert_array_equal(model.extend(X[rows]).vectors, host.vectors[rows])


# ------------------------------------------------------------------------------------ 4. workgroup and block edges
@pytest.mark.parametrize("kernel", ["lae", "se"])
def test_workgroup_and_row_block_edges(kernel):
    import torch
    n, d, s, r, K = SHAPES["A"]
    X = case("A")[0]
    model, pair, host = fitted("A", kernel, "cluster-normalized", True)
    L = _lib.lib()
    for n_new in (1, 255, 256, 257, 513, 600):
        rows = some_rows(n, n_new, seed=n_new)
        want = host.vectors[rows]
        L.flgp_set_tuning(b"model_extend_block", 256)
        try:
            small = model.extend(X[rows]).vectors
            res = model.extend(X[rows], resident=True)
            # the device-pointer entry, on padded buffers: ldx = n_new + 3, ldv = n_new + 5, NaN around
            dX = torch.full((d, n_new + 3), float("nan"), dtype=torch.float64, device=DEV)
            dX[:, :n_new] = torch.from_numpy(np.ascontiguousarray(X[rows].T)).to(DEV)
            out = torch.full((K + 1, n_new + 5), float("nan"), dtype=torch.float64, device=DEV)
            st = torch.cuda.current_stream().cuda_stream
            _lib.check(L.flgp_dev_spectrum_model_extend(st, model._h, dX.data_ptr(), n_new, n_new + 3, out.data_ptr(), n_new + 5))
            torch.cuda.synchronize()
        finally:
            L.flgp_set_tuning(b"model_extend_block", 1 << 20)
        np.testing.assert_array_equal(small, want)
        assert (res.n, res.K) == (n_new, K)
        np.testing.assert_array_equal(res.to_host().vectors, want)
        out = out.cpu().numpy()
        np.testing.assert_array_equal(out[:K, :n_new].T, want)
        assert np.isnan(out[K]).all() and np.isnan(out[:, n_new:]).all()
        np.testing.assert_array_equal(model.extend(X[rows]).vectors, small)          # the default block: the same bits
    L.flgp_set_tuning(b"model_extend_block", 7)                                       # below 256: raised to 256
    try:
        rows = some_rows(n, 300, seed=9)
        np.testing.assert_array_equal(model.extend(X[rows]).vectors, host.vectors[rows])
    finally:
        L.flgp_set_tuning(b"model_extend_block", 1 << 20)


# ------------------------------------------------------------------------------------------------- 5. new rows (LAE)
@pytest.mark.parametrize("shape,gl,root", [("A", "rw", False), ("A", "normalized", True), ("A", "cluster-normalized", False),
                                           ("A", "cluster-normalized", True), ("B", "cluster-normalized", True),
                                           ("wide", "normalized", False)])
def test_new_rows_are_the_restatement_bit_for_bit(oracle, shape, gl, root):
    n, d, s, r, K = SHAPES[shape]
    U0 = case(shape)[1]
    model, pair, host = fitted(shape, "lae", gl, root)
    X2 = synth.gaussian_mixture(517, d, components=5, seed=n + d + 1000)              # another draw: none of the fit rows
    h = model.to_host()
    want, values = npm.extend(X2, U0, r, gl, h["colsum_gl"], h["colsum_spectrum"], h["sizes"], h["V"], h["eig"], n, root)
    ep = model.extend(X2)
    np.testing.assert_array_equal(ep.vectors, want)
    np.testing.assert_array_equal(ep.values, values)
    np.testing.assert_array_equal(ep.values, host.values)
    assert np.isfinite(want).all() and np.abs(want).max() > 0.0


# ------------------------------------------------------------------------------------- 6. flgp_dev_extend_scale alone
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("r", [1, 2, 10, 32])
def test_extend_scale_is_the_three_passes(n, r):
    import torch
    s = 48
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    idx, val, sizes = nps.ell_inputs(n, s, r, seed=17)
    rng = np.random.default_rng([n, r])
    c1 = rng.uniform(0.5, 30.0, size=s); c1[5] = 0.0; c1[11] = -3.25            # |c| matters only in the last pass,
    c2 = rng.uniform(0.5, 30.0, size=s); c2[7] = 0.0; c2[13] = -2.5             # but both take a zero and a negative sum
    idx[0, 0] = min(idx[0, 0], 5)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    d_idx, d_c1, d_c2, d_nc = dev(idx), dev(c1), dev(c2), dev(sizes)
    for use_c1, use_nc in ((True, True), (True, False), (False, False), (False, True)):
        want = npm.scale(idx, val, c1 if use_c1 else None, sizes if use_nc else None, c2)
        one = dev(val)
        _lib.check(L.flgp_dev_extend_scale(st, d_idx.data_ptr(), one.data_ptr(), n, r, d_c1.data_ptr() if use_c1 else None,
                                           d_nc.data_ptr() if use_nc else None, d_c2.data_ptr()))
        three = dev(val)
        if use_c1:
            _lib.check(L.flgp_dev_col_scale(st, d_idx.data_ptr(), three.data_ptr(), n, r, d_c1.data_ptr(),
                                            d_nc.data_ptr() if use_nc else None, 0))
        _lib.check(L.flgp_dev_row_normalize(st, three.data_ptr(), n, r))
        _lib.check(L.flgp_dev_col_scale(st, d_idx.data_ptr(), three.data_ptr(), n, r, d_c2.data_ptr(), None, 1))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(one.cpu().numpy(), want)
        np.testing.assert_array_equal(three.cpu().numpy(), want)
    np.testing.assert_array_equal(d_idx.cpu().numpy(), idx)                         # the pattern is read only


# --------------------------------------------------------------------------------------------------------- 7. serving
@pytest.mark.parametrize("m,shape", [(50, "As"), (120, "A")])
def test_serving_pair_feeds_the_consumers(m, shape):
    """rows [0, m) of the fit as the head, the next 64 fit rows extended behind them: the stacked fit rows bit for bit, and
    the consumers agree with the fit's own pair to 1e-12 of the result's scale (the inputs are identical, only the leading
    dimension differs: summation order over K <= 200 terms, about 2e-14).  m = 50 < K = s = 200 takes the consumers' m <= K
    branch, m = 120 > K = 20 the Woodbury one."""
    n, d, s, r, K = SHAPES[shape]
    X = case(shape)[0]
    model, pair, host = fitted(shape, "lae", "cluster-normalized", True)
    both = model.extend(X[m:m + 64], resident=True, head=pair, head_rows=np.arange(m))
    assert (both.n, both.K) == (m + 64, K)
    got = both.to_host()
    np.testing.assert_array_equal(got.vectors, host.vectors[:m + 64])
    np.testing.assert_array_equal(got.values, host.values)
    rng = np.random.default_rng(m)
    Y = np.sin(X[:m, :1] * 2.0) + 0.1 * rng.normal(size=(m, 1))
    idx0, idx1 = np.arange(m), m + np.arange(64)
    a = both.predict_regression_cpp(Y, idx0, idx1, K, (2.0, 0.1), 1e-5)
    b = pair.predict_regression_cpp(Y, idx0, idx1, K, (2.0, 0.1), 1e-5)
    assert np.abs(b).max() > 0.0
    assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    Yc = (X[:m, 0] > np.median(X[:m, 0])).astype(float)
    pa = both.posterior_distribution_classification(idx0, idx1, K, 2.0, Yc, 1e-3, 1e-3)
    pb = pair.posterior_distribution_classification(idx0, idx1, K, 2.0, Yc, 1e-3, 1e-3)
    for key in ("mean", "cov"):
        assert np.abs(pb[key]).max() > 0.0
        assert np.abs(pa[key] - pb[key]).max() <= 1e-12 * np.abs(pb[key]).max()
    # shuffled head rows and no head at all
    hr = some_rows(n, 33, seed=m)
    sh = model.extend(X[:5], resident=True, head=pair, head_rows=hr).to_host()
    np.testing.assert_array_equal(sh.vectors, np.vstack([host.vectors[hr], host.vectors[:5]]))
    np.testing.assert_array_equal(model.extend(X[:5], resident=True).to_host().vectors, host.vectors[:5])


# ------------------------------------------------------------------------------- 8. repeatability, free, live refusals
def test_two_calls_give_the_same_bits_and_free_twice_is_harmless():
    n, d, s, r, K = SHAPES["B"]
    X, U0, U = case("B")
    X2 = synth.gaussian_mixture(100, d, components=5, seed=77)
    model, pair = api.heat_kernel_spectrum_model(X, X[:0], s, r, 12, models={"kernel": "se", "gl": "normalized"}, epsilon=0.7, U=U)
    a = model.extend(X2).vectors; b = model.extend(X2).vectors
    np.testing.assert_array_equal(a, b)
    model2, _ = api.heat_kernel_spectrum_model(X, X[:0], s, r, 12, models={"kernel": "se", "gl": "normalized"}, epsilon=0.7, U=U)
    np.testing.assert_array_equal(model2.extend(X2).vectors, a)
    model.free(); model.free()
    with pytest.raises(ValueError, match="freed"):
        model.extend(X2)
    assert pair.to_host().vectors.shape == (n, 12)                                   # the pair outlives the model


def test_refusals_with_live_handles():
    n, d, s, r, K = SHAPES["B"]
    X = case("B")[0]
    model, pair, host = fitted("B", "lae", "cluster-normalized", True)
    other = fitted("A", "lae", "cluster-normalized", True)[1]                        # K = 20, the model's is 40
    L = _lib.lib()
    Xf = np.asfortranarray(X[:8])
    out = ctypes.c_void_p(1)
    rows = np.array([0, 1, n], dtype=np.int32)

    def refused(rc, what):
        assert rc == -1 and what in L.flgp_last_error().decode(), L.flgp_last_error()
        assert out.value is None
        out.value = 1
    refused(L.flgp_spectrum_model_extend_resident(model._h, Xf.ctypes.data, 8, pair._h, rows.ctypes.data, 3, ctypes.byref(out)),
            "head_rows[2]=%d out of range" % n)
    rows[2] = -1
    refused(L.flgp_spectrum_model_extend_resident(model._h, Xf.ctypes.data, 8, pair._h, rows.ctypes.data, 3, ctypes.byref(out)),
            "head_rows[2]=-1 out of range")
    refused(L.flgp_spectrum_model_extend_resident(model._h, Xf.ctypes.data, 8, other._h, rows.ctypes.data, 2, ctypes.byref(out)),
            "K = 20, the model K = 40")
    refused(L.flgp_spectrum_model_extend_resident(model._h, Xf.ctypes.data, 8, pair._h, None, 2, ctypes.byref(out)), "head_rows")
    bad = Xf.copy(order="F"); bad[3, 1] = np.nan
    refused(L.flgp_spectrum_model_extend_resident(model._h, bad.ctypes.data, 8, None, None, 0, ctypes.byref(out)), "NA / NaN / Inf")
    with pytest.raises(api.FlgpError, match="NA / NaN / Inf"):
        model.extend(np.where(np.arange(8)[:, None] == 2, np.inf, X[:8]))
    # K = s with an anchor that no point chose reaches into the null space (test_unusable_spectrum_is_refused_on_every_path):
    # refused at the fit as the resident entry refuses it, both handles cleared
    U = case("B")[2].copy(order="F"); U[7, :d] = 1e6
    Xf = np.asfortranarray(X)
    hm = ctypes.c_void_p(1); hp = ctypes.c_void_p(1); hr = ctypes.c_void_p(1)
    rc = L.flgp_heat_kernel_spectrum_model(Xf.ctypes.data, n, d, U.ctypes.data, s, d + 1, r, s, b"lae", b"rw", 1, 0.1,
                                           ctypes.byref(hm), ctypes.byref(hp))
    msg = L.flgp_last_error()
    rc2 = L.flgp_heat_kernel_spectrum_resident(Xf.ctypes.data, n, d, U.ctypes.data, s, d + 1, r, s, b"lae", b"rw", 1, 0.1, ctypes.byref(hr))
    assert rc == rc2 == -5 and msg == L.flgp_last_error() and b"null space" in msg
    assert hm.value is None and hp.value is None and hr.value is None
