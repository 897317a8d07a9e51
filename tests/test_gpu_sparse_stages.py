"""GPU (-m gpu): the sparse device stages between the k-NN list and the heat kernel, each called with known inputs at
its tile, stride and r edges and compared bit for bit (`assert_array_equal`) with the plain numpy restatements of
tests/np_sparse_stages.py or with the compiled oracle; tests/test_sparse_stage_restatements.py ties the two together on
the CPU.  Only the exp()-dependent SE weights get a tolerance: 4 ulp, the project's bar for them (test_gpu_parity.py).

U-recovery (flgp_dev_u_recover, csrc/sparse.hip) goes through ctypes, because HipStages hides ldv, ldo, the optional
workspace and the optional values pointer: V sits in a buffer with ldv = s + 3 whose pad is NaN, the output in one with
ldo = n + 5 and a column too many, all NaN beforehand, and every element outside n x K must still be NaN afterwards."""
import functools
import math

import numpy as np
import pytest
import torch

import np_sparse_stages as nps
from conftest import make_case
from flgp_amd import _lib, api
from flgp_amd.pipeline import HipStages

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLGP_OK, FLGP_ERR_INVALID = 0, -1


@pytest.fixture(scope="module")
def stages():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    return HipStages(DEV)


def cm(a, dtype=torch.float64):
    """(n x k) array -> column-major device tensor of shape (k, n)."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).T)).to(dtype).to(DEV)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def nan_buffer(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)


# ============================================================================================================ U-recovery
def run_u_recover(stages, idx, val, V, eig, scale, root, workspace=True, want_values=True, n=None, r=None, K=None, ldo=None):
    """flgp_dev_u_recover on padded buffers.  Returns (rc, vectors buffer (K + 1, ldo), values buffer (K + 1) or None);
    n, r, K and ldo override what the arrays say (for the refusals: the buffers keep their true size)."""
    n0, r0 = idx.shape
    s, K0 = V.shape
    ldv, ldo0 = s + 3, n0 + 5
    dV = nan_buffer(K0, ldv)
    dV[:, :s] = cm(V)
    out = nan_buffer(K0 + 1, ldo0)
    values = nan_buffer(K0 + 1) if want_values else None
    d_idx = dev(idx) if n0 else torch.zeros((1, r0), dtype=torch.int32, device=DEV)
    d_val = dev(val) if n0 else torch.zeros((1, r0), dtype=torch.float64, device=DEV)
    d_eig = dev(eig)
    work = stages.empty((stages.L.flgp_dev_u_recover_workspace(s, K0) // 8 + 1,)) if workspace else None
    rc = stages.L.flgp_dev_u_recover(stages._st(), d_idx.data_ptr(), d_val.data_ptr(), n0 if n is None else n,
                                     r0 if r is None else r, dV.data_ptr(), ldv, s, d_eig.data_ptr(), K0 if K is None else K,
                                     float(scale), int(root), out.data_ptr(), ldo0 if ldo is None else ldo,
                                     values.data_ptr() if want_values else None, work.data_ptr() if workspace else None)
    stages.sync()
    return rc, out.cpu().numpy(), (values.cpu().numpy() if want_values else None)


def check_u_recover(stages, idx, val, V, eig, scale, root, workspace=True, want_values=True):
    n, r = idx.shape
    K = V.shape[1]
    rc, out, values = run_u_recover(stages, idx, val, V, eig, scale, root, workspace, want_values)
    assert rc == FLGP_OK, stages.L.flgp_last_error()
    ref, ref_values = nps.u_recover(idx, val, V, eig, scale, root=bool(root))
    np.testing.assert_array_equal(out[:K, :n], ref.T)                       # bit for bit
    assert np.isnan(out[:K, n:]).all(), "rows past n were written"
    assert np.isnan(out[K]).all(), "a column past K was written"
    if want_values:
        np.testing.assert_array_equal(values[:K], ref_values)
        assert np.isnan(values[K]), "values past K were written"
    return out[:K, :n], (values[:K] if want_values else None)


@pytest.mark.parametrize("case", nps.U_RECOVER_CASES, ids=[nps.u_recover_case_id(c) for c in nps.U_RECOVER_CASES])
def test_u_recover_bit_exact(stages, case):
    """Each of the four kernels behind the entry point at, one below and one above its column tile and its row block, with
    a second column tile, r from 1 to FLGP_RMAX, s around transpose_v_kernel's 32-wide tile, both `root` settings, a scale
    that is a power of two only by accident, and once per kernel without the values output."""
    route, K, n, r, s, root, scale, want_values, seed = case
    assert route == nps.u_recover_route(K, route != "null")
    idx, val, V, eig = nps.u_recover_inputs(K, n, r, s, seed)
    check_u_recover(stages, idx, val, V, eig, nps.u_recover_scale(scale, n), root, workspace=route != "null",
                    want_values=want_values)


def test_u_recover_routes_agree(stages):
    """One input through all four kernels: K = 8 with (KPL = 4) and without a workspace, and its leading 7 (tiled) and 6
    (KPL = 2) columns as runs of their own on the leading columns of V."""
    K, n, r, s = 8, 300, 10, 97
    idx, val, V, eig = nps.u_recover_inputs(K, n, r, s, 3)
    scale = math.sqrt(n)
    wide, _ = check_u_recover(stages, idx, val, V, eig, scale, 1, workspace=True)
    plain, _ = check_u_recover(stages, idx, val, V, eig, scale, 1, workspace=False)
    np.testing.assert_array_equal(plain, wide)
    for Kc in (7, 6):
        Vc = np.asfortranarray(V[:, :Kc])
        lead, _ = check_u_recover(stages, idx, val, Vc, eig[:Kc].copy(), scale, 1, workspace=True)
        np.testing.assert_array_equal(lead, wide[:Kc])
        lead0, _ = check_u_recover(stages, idx, val, Vc, eig[:Kc].copy(), scale, 1, workspace=False)
        np.testing.assert_array_equal(lead0, wide[:Kc])


@pytest.mark.parametrize("route,K,n", [("null", 17, 300), ("tiled", 129, 70), ("kpl2", 258, 70), ("kpl4", 516, 40)])
def test_u_recover_zero_sigma_columns(stages, route, K, n):
    """sigma == 0 (an exact 0.0, a negative eigenvalue, -0.0) in the first and in a later column tile of each kernel: the
    column is exactly +0.0 -- not Inf, NaN or -0.0 -- and `values` is +0.0 there for both `root` settings; every other
    column is the restatement's.  Called directly: HipStages.u_recover refuses such a spectrum before it gets here."""
    r, s = 10, 33
    idx, val, V, eig = nps.u_recover_inputs(K, n, r, s, 4)
    dead = np.array([1, 2, 3, K - 3, K - 2, K - 1])
    eig[dead] = [0.0, -0.25, -0.0, -0.0, 0.0, -1e-300]
    for root in (0, 1):
        out, values = check_u_recover(stages, idx, val, V, eig, 1000.0 / 3.0, root, workspace=route != "null")
        assert (out[dead] == 0.0).all() and not np.signbit(out[dead]).any()
        assert (values[dead] == 0.0).all() and not np.signbit(values[dead]).any()
        live = np.setdiff1d(np.arange(K), dead)
        assert np.isfinite(out[live]).all() and (np.abs(out[live]).max(axis=1) > 0).all()


@pytest.mark.parametrize("workspace", [True, False])
def test_u_recover_no_rows(stages, workspace):
    """n == 0: FLGP_OK, `values` filled, `vectors` untouched"""
    K, r, s = 6, 3, 31
    idx, val, V, eig = nps.u_recover_inputs(K, 0, r, s, 0)
    for root in (0, 1):
        rc, out, values = run_u_recover(stages, idx, val, V, eig, 2.0, root, workspace=workspace)
        assert rc == FLGP_OK
        assert np.isnan(out).all()
        np.testing.assert_array_equal(values[:K], np.sqrt(eig) if root else eig)
        assert np.isnan(values[K])


@pytest.mark.parametrize("bad", [dict(r=0), dict(r=33), dict(K=0), dict(ldo=9)])
def test_u_recover_refusals(stages, bad):
    """r outside 1..FLGP_RMAX, K = 0 and ldo < n: FLGP_ERR_INVALID with a message, and nothing is launched"""
    K, n, r, s = 6, 10, 3, 31
    idx, val, V, eig = nps.u_recover_inputs(K, n, r, s, 0)
    for workspace in (True, False):
        rc, out, values = run_u_recover(stages, idx, val, V, eig, 2.0, 1, workspace=workspace, **bad)
        assert rc == FLGP_ERR_INVALID
        assert b"u_recover" in stages.L.flgp_last_error()
        assert np.isnan(out).all() and np.isnan(values).all()


# ================================================================================================== r up to FLGP_RMAX
@pytest.mark.parametrize("r,d", [(21, 2), (24, 16), (25, 3), (25, 16), (32, 2), (32, 16), (32, 64), (32, 100), (28, 72)])
def test_lae_bit_exact_up_to_rmax(oracle, r, d):
    """Beyond r = 20: the LDS kernel gives up lanes from r = 25 (nt = 16) and reads the anchors from memory for d > 64.
    As test_lae_bit_exact of test_gpu_parity.py, with its forced two-pass settings."""
    n, s = 500, 64
    X, U0, _ = make_case(n, d, s, r, seed=31 * r + d, with_sizes=False)
    ei, ev = oracle.lae(X, U0, r)
    Z = api.LAE_cpp(X, U0, r)
    np.testing.assert_array_equal(Z.indptr, np.arange(0, n * r + 1, r))
    np.testing.assert_array_equal(Z.indices.reshape(n, r), ei)
    np.testing.assert_array_equal(Z.data.reshape(n, r), ev)
    L = _lib.lib()
    L.flgp_set_tuning(b"lae_cut_min_n", 0)
    try:
        for cut in (1, 7, 40):
            L.flgp_set_tuning(b"lae_cut", cut)
            Z2 = api.LAE_cpp(X, U0, r)
            np.testing.assert_array_equal(Z2.indices.reshape(n, r), ei)
            np.testing.assert_array_equal(Z2.data.reshape(n, r), ev)
    finally:
        L.flgp_set_tuning(b"lae_cut_min_n", 32768)
        L.flgp_set_tuning(b"lae_cut", 13)


@functools.lru_cache(maxsize=None)
def _laplacian_case(n, r):
    """points, anchors with sizes and the oracle's un-normalised LAE matrix, computed once for the three gl modes"""
    from oracle import flgp_oracle as O
    d, s = 3, 48
    X, U0, U = make_case(n, d, s, r, seed=n + r)
    ei, zl = O.lae(X, U0, r)
    for a in (X, U0, U, ei, zl):
        a.setflags(write=False)
    return X, U0, U, ei, zl


@pytest.mark.parametrize("gl", ["rw", "normalized", "cluster-normalized"])
@pytest.mark.parametrize("n", [255, 256, 257, 700])
@pytest.mark.parametrize("r", [24, 25, 32])
def test_laplacian_bit_exact_up_to_rmax(oracle, gl, n, r):
    """row_normalize_kernel holds 256 rows x r doubles in LDS: more than 48 KB from r = 25, around its 256-row block"""
    d, s = 3, 48
    X, U0, U, ei, zl = _laplacian_case(n, r)
    zn = oracle.graph_laplacian(ei, zl, s, gl, U[:, d])
    Z = api.cross_similarity_lae_cpp(X, U, r, gl)
    np.testing.assert_array_equal(Z.indices.reshape(n, r), ei)
    np.testing.assert_array_equal(Z.data.reshape(n, r), zn)
    Zl = api.LAE_cpp(X, U0, r)
    np.testing.assert_array_equal(Zl.data.reshape(n, r), zl)
    np.testing.assert_array_equal(api.graphLaplacian_cpp(Zl, gl, U[:, d]).data.reshape(n, r), zn)


@pytest.mark.parametrize("with_sizes", [False, True])
@pytest.mark.parametrize("r", [1, 24, 25, 32])
def test_col_scale_and_row_normalize_stages(oracle, stages, r, with_sizes):
    """col_scale(mode 0) followed by row_normalize, and the fused col_scale_row_normalize: the same bits, and the
    restatement's; col_scale(mode 1) likewise.  n = 700: two full 256-row blocks and a ragged one."""
    n, s = 700, 48
    idx, val, sizes = nps.ell_inputs(n, s, r, seed=5)
    nc = sizes if with_sizes else None
    c = nps.colsum(idx, val, s)
    d_idx = dev(idx); d_c = dev(c); d_nc = dev(nc) if with_sizes else None
    scaled = nps.col_scale(idx, val, c, nc, 0)
    want = nps.row_normalize(scaled)
    two = dev(val)
    stages.col_scale(d_idx, two, d_c, d_nc, 0)
    np.testing.assert_array_equal(two.cpu().numpy(), scaled)
    stages.row_normalize(two)
    np.testing.assert_array_equal(two.cpu().numpy(), want)
    one = dev(val)
    stages.col_scale_row_normalize(d_idx, one, d_c, d_nc)
    np.testing.assert_array_equal(one.cpu().numpy(), want)
    np.testing.assert_array_equal(want, oracle.graph_laplacian(idx, val, s, "cluster-normalized" if with_sizes else "normalized", nc))
    alone = dev(val)
    stages.row_normalize(alone)
    np.testing.assert_array_equal(alone.cpu().numpy(), nps.row_normalize(val))
    a = dev(val)
    stages.col_scale(d_idx, a, d_c, d_nc, 1)                    # mode 1 ignores num_class
    np.testing.assert_array_equal(a.cpu().numpy(), nps.col_scale(idx, val, c, None, 1))
    np.testing.assert_array_equal(d_idx.cpu().numpy(), idx)     # the pattern is read only


@pytest.mark.parametrize("n,s", [(700, 40), (2049, 65)])
@pytest.mark.parametrize("r", [16, 17, 31, 32])
def test_colsum_and_gram_up_to_rmax(oracle, stages, n, s, r):
    """gram_kernel<16,*> serves r <= 16 and gram_kernel<32,*> the rest, two rows per group at r = 32; n = 2049 crosses the
    1024-row chunks of the column sums twice.  Once with all columns in one LDS table, once by windows of 16."""
    idx, val, _ = nps.ell_inputs(n, s, r, seed=11)
    d_idx = dev(idx); d_val = dev(val)
    want_c = oracle.colsum(idx, val, s)
    want_G = oracle.gram(idx, val, s)
    csc = stages.csc(d_idx, s)
    np.testing.assert_array_equal(stages.colsum(d_idx, d_val, s).cpu().numpy(), want_c)
    G = stages.gram(d_idx, d_val, csc).cpu().numpy()
    np.testing.assert_array_equal(G, want_G)
    np.testing.assert_array_equal(G, G.T)
    stages.L.flgp_set_tuning(b"sparse_window", 16)
    try:
        cw = stages.colsum(d_idx, d_val, s).cpu().numpy()
        Gw = stages.gram(d_idx, d_val, csc).cpu().numpy()
    finally:
        stages.L.flgp_set_tuning(b"sparse_window", 0)
    np.testing.assert_array_equal(cw, want_c)
    np.testing.assert_array_equal(Gw, want_G)


# =================================================================================================== SE weights and mean
TINY = 2.0 ** -1022          # the smallest normal double


def assert_within_4ulp(got, ref):
    """4 ulp of the reference; where the reference is subnormal (or zero) an absolute 2^-1022 instead"""
    tol = np.where(np.abs(ref) < TINY, TINY, 4.0 * np.spacing(np.abs(ref)))
    bad = ~(np.abs(got - ref) <= tol)
    assert not bad.any(), (got[bad][:4], ref[bad][:4])


def run_se_weights(stages, fn, kidx, kdist, width):
    """an SE entry point on k-NN lists held with ldk = n + 7 (the pad: index 0, distance NaN); the ELL output has a row
    too many, which must stay untouched"""
    r, n = kidx.shape
    ldk = n + 7
    bi = torch.zeros((r, ldk), dtype=torch.int32, device=DEV); bi[:, :n] = kidx
    bd = nan_buffer(r, ldk); bd[:, :n] = kdist
    ei = torch.full((n + 1, r), -7, dtype=torch.int32, device=DEV)
    ev = nan_buffer(n + 1, r)
    rc = fn(stages._st(), bi.data_ptr(), bd.data_ptr(), n, ldk, r, float(width), ei.data_ptr(), ev.data_ptr())
    stages.sync()
    assert rc == FLGP_OK, stages.L.flgp_last_error()
    ei = ei.cpu().numpy(); ev = ev.cpu().numpy()
    assert (ei[n] == -7).all() and np.isnan(ev[n]).all(), "a row past n was written"
    return ei[:n], ev[:n]


@functools.lru_cache(maxsize=None)
def _se_cloud():
    X, U0, _ = make_case(300, 3, 40, 6, seed=21, with_sizes=False)
    return np.asfortranarray(X + 0.05), U0        # the anchors are rows of the cloud: shifted, so that no distance is 0


@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("r", [1, 2, 6, 32])
def test_se_weights_against_the_oracle(oracle, stages, r, n):
    """The sorted insertion of se_weights_kernel at r = 1 and r = FLGP_RMAX, around its 256-row block, with ldk > n; three
    bandwidths: an ordinary one, one so small that weights underflow (dist / den > 746: exactly 0.0 on both sides,
    subnormal results on the way there), and one so large that every weight is 1 - O(1e-12)."""
    X, U0 = _se_cloud()
    anchors = stages.anchor_prep(cm(U0))
    kidx, kdist = stages.knn(cm(X[:n]), anchors, r, want_dist=True)
    hi = kidx.cpu().numpy().T; hd = kdist.cpu().numpy().T                   # n x r
    dmax = float(hd.max())
    assert dmax > 0
    eps_under = math.sqrt(dmax / 800.0 / 4.0)                                # den = dmax / 800: the farthest neighbour underflows
    eps_one = math.sqrt(dmax * 1e12 / 4.0)                                   # dist / den <= 1e-12
    for eps in (0.5, eps_under, eps_one):
        oi, ov = oracle.se_weights(hi, hd, eps)
        ei, ev = run_se_weights(stages, stages.L.flgp_dev_se_weights, kidx, kdist, eps)
        np.testing.assert_array_equal(ei, oi)
        assert (np.diff(ei, axis=1) > 0).all()                               # strictly ascending columns per row
        assert_within_4ulp(ev, ov)
        den = (4.0 * eps) * eps
        order = np.argsort(hi, axis=1, kind="stable")
        gone = np.take_along_axis(hd, order, axis=1) / den > 746.0
        assert (ev[gone] == 0.0).all() and (ov[gone] == 0.0).all()
        if eps == eps_under:
            assert gone.any()
        if eps == eps_one:
            assert (ev <= 1.0 + 1e-15).all() and (1.0 - ev).max() < 2e-12 and (ov < 1.0).any()
        di, dv = run_se_weights(stages, stages.L.flgp_dev_se_weights_den, kidx, kdist, den)
        np.testing.assert_array_equal(di, ei)
        np.testing.assert_array_equal(dv, ev)                                # the same kernel on the same den: the same bits


def test_se_weights_refusals(stages):
    i = torch.zeros((1, 8), dtype=torch.int32, device=DEV); x = nan_buffer(1, 8)
    oi = torch.zeros((8, 1), dtype=torch.int32, device=DEV); ov = nan_buffer(8, 1)
    for fn in (stages.L.flgp_dev_se_weights, stages.L.flgp_dev_se_weights_den):
        for n, ldk, r in ((8, 7, 1), (8, 8, 0), (8, 8, 33)):
            assert fn(stages._st(), i.data_ptr(), x.data_ptr(), n, ldk, r, 1.0, oi.data_ptr(), ov.data_ptr()) == FLGP_ERR_INVALID
            assert b"SE weights" in stages.L.flgp_last_error()
    stages.sync()
    assert np.isnan(ov.cpu().numpy()).all()


@pytest.mark.parametrize("count", nps.MEAN_COUNTS)
def test_mean_is_the_fixed_tree(stages, count):
    """flgp_dev_mean at, below and above its 256-lane stride and its 4096-element slab: the bits of the restated tree,
    twice in a row"""
    x = nps.mean_inputs(count)
    want = nps.mean(x)
    assert abs(want - math.fsum(x) / count) <= count * 2.0 ** -53 * np.abs(x).max()
    buf = nan_buffer(count + 1); buf[:count] = dev(x)
    nparts = (count + 4095) // 4096
    got = []
    for _ in range(2):
        out = nan_buffer(2); work = nan_buffer(nparts + 1)
        assert stages.L.flgp_dev_mean(stages._st(), buf.data_ptr(), count, out.data_ptr(), work.data_ptr()) == FLGP_OK
        stages.sync()
        o = out.cpu().numpy(); w = work.cpu().numpy()
        assert np.isnan(o[1]) and np.isnan(w[nparts]) and np.isfinite(w[:nparts]).all()
        got.append(o[:1].copy())
    np.testing.assert_array_equal(got[0], np.array([want]))
    np.testing.assert_array_equal(got[1], got[0])


def test_mean_of_nothing_is_refused(stages):
    out = nan_buffer(1); work = nan_buffer(1); x = nan_buffer(1)
    assert stages.L.flgp_dev_mean(stages._st(), x.data_ptr(), 0, out.data_ptr(), work.data_ptr()) == FLGP_ERR_INVALID
    assert b"mean" in stages.L.flgp_last_error()
    stages.sync()
    assert np.isnan(out.cpu().numpy()).all()
