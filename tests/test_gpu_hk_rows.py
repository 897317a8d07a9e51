"""GPU (-m gpu): flgp_dev_hk_rows (csrc/sparse.hip), the heat-kernel covariance from the sparse rows,
    H(i, b) = sum_a val(i, a) Wm(idx(i, a), b),   Wm = (Vs diag(scale / sigma)) (V1 diag(w))^T,
checked two ways on every shape: bit for bit against the numpy restatement (tests/np_hk_rows.py: B and Vw rounded products,
Wm a k-ascending fma chain, H multiply-then-add over a ascending), and within 1e-8 max|H| of flgp_dev_u_recover +
flgp_dev_hk on the same inputs.  The device's exp may differ from numpy's in the last bit, so the weights w_k the
restatement uses are the device's own, read through flgp_dev_hk on identity blocks (H = I diag(w) I^T is exact), and held
to numpy's within two units in the last place.

Shapes: the smallest n the LDS row kernel takes (10000; 9999 is refused by the route query), s on both sides of every
slice-width change (W = 4 | 3 | 3 | 2 | 2 | 1 | 1 at 5120 | 5121 | 6826 | 6827 | 10240 | 10241 | 20480; none at 20481), m off
and on a multiple of W and more than one slice per range, K = 1, 7, 200, r = 1, 3, 10, 11, 32 with n r odd twice, every
leading dimension larger than its extent with NaN around everything."""
import functools
import math

import numpy as np
import pytest
import torch

import np_hk_rows as R
from conftest import make_case
from flgp_amd import _lib
from flgp_amd.pipeline import HipStages

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H_RTOL = 1e-8
T = 10.0

#        n      s     m    K   r
CASES = [
    (10000, 5120, 8, 200, 10),
    (10000, 5121, 5, 7, 10),
    (10000, 6826, 3, 7, 1),
    (10000, 6827, 4, 7, 32),
    (10000, 10240, 1, 1, 10),
    (10001, 10241, 5, 7, 3),
    (10000, 20480, 3, 7, 10),
    (10001, 5000, 1001, 7, 11),
    (10000, 64, 4, 200, 10),
]
IDS = ["n%d-s%d-m%d-K%d-r%d" % c for c in CASES]


def test_the_cases_take_every_width_and_edge():
    assert [R.slice_width(c[1]) for c in CASES[:7]] == [4, 3, 3, 2, 2, 1, 1]
    assert {c[2] for c in CASES} >= {1, 3, 4, 5, 8, 1001} and {c[3] for c in CASES} == {1, 7, 200}
    assert {c[4] for c in CASES} >= {1, 10, 32} and sum((c[0] * c[4]) % 2 for c in CASES) >= 2


@pytest.fixture(scope="module")
def stages():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    return HipStages(DEV)


@pytest.fixture()
def knob(stages):
    """sets hk_rows and puts the default back"""
    def set_(v):
        stages.L.flgp_set_tuning(b"hk_rows", v)
    yield set_
    stages.L.flgp_set_tuning(b"hk_rows", 1)


@functools.lru_cache(maxsize=None)
def inputs(n, s, m, K, r, dead=None):
    """(idx, val, Vs, eig, values, V1) -- read-only, shared.  The rows name about 300 of the s anchors, the first and the
    last among them (the restatement forms Wm for those alone); val = normal x 10**uniform(-3, 3): mixed signs and
    magnitudes, so that another order of the sum changes bits."""
    rng = np.random.default_rng([n, s, m, K, r])
    used = np.unique(np.concatenate([[0, s - 1], rng.integers(0, s, 300)]))
    idx = used[rng.integers(0, used.size, size=(n, r))].astype(np.int32)
    idx[0, 0] = 0; idx[n - 1, r - 1] = s - 1
    val = rng.normal(size=(n, r)) * 10.0 ** rng.uniform(-3.0, 3.0, size=(n, r))
    Vs = rng.normal(size=(s, K)); V1 = rng.normal(size=(m, K))
    eig = np.sort(rng.uniform(0.05, 1.0, size=K))[::-1].copy()
    if dead is not None:
        eig[dead] = 0.0
    values = np.sqrt(eig)
    for a in (idx, val, Vs, eig, values, V1):
        a.setflags(write=False)
    return idx, val, Vs, eig, values, V1


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def padded(a, ld):
    """a (rows x cols) as a column-major block of leading dimension ld inside NaN"""
    t = torch.full((a.shape[1], ld), float("nan"), dtype=torch.float64, device=DEV)
    t[:, :a.shape[0]] = dev(np.ascontiguousarray(np.asarray(a).T))
    return t


def device_weights(stages, values, t):
    K = values.size
    eye = torch.eye(K, dtype=torch.float64, device=DEV)
    w = torch.diagonal(stages.hk(dev(values), t, eye, eye)).cpu().numpy().copy()
    wn = R.weights(values, t)
    assert (np.abs(w - wn) <= 2.0 * np.spacing(wn)).all()
    return w


def run_hk_rows(stages, idx, val, Vs, eig, scale, values, t, V1):
    n, r = idx.shape
    s, K = Vs.shape
    m = V1.shape[0]
    L = stages.L
    ldv, ld1, ldh = s + 3, m + 2, n + 5
    dVs, dV1 = padded(Vs, ldv), padded(V1, ld1)
    H = torch.full((m + 1, ldh), float("nan"), dtype=torch.float64, device=DEV)
    work = stages.empty((L.flgp_dev_hk_rows_workspace(s, m, K) // 8 + 1,))
    d_idx, d_val, d_eig, d_values = dev(idx), dev(val), dev(eig), dev(values)
    rc = L.flgp_dev_hk_rows(stages._st(), d_idx.data_ptr(), d_val.data_ptr(), n, r, dVs.data_ptr(), ldv, s, d_eig.data_ptr(), K,
                            float(scale), d_values.data_ptr(), float(t), dV1.data_ptr(), ld1, m, H.data_ptr(), ldh, work.data_ptr())
    stages.sync()
    assert rc == 0, L.flgp_last_error()
    H = H.cpu().numpy()
    assert np.isnan(H[:m, n:]).all(), "rows past n were written"
    assert np.isnan(H[m]).all(), "a column past m was written"
    return H[:m, :n].T


def run_old_route(stages, idx, val, Vs, eig, scale, values, t, V1):
    """flgp_dev_u_recover + flgp_dev_hk on the same inputs (n x m)"""
    n, r = idx.shape
    s, K = Vs.shape
    L = stages.L
    d_idx, d_val, d_eig = dev(idx), dev(val), dev(eig)
    dVs = dev(np.ascontiguousarray(Vs.T))
    vectors = stages.empty((K, n))
    work = stages.empty((L.flgp_dev_u_recover_workspace(s, K) // 8 + 1,))
    _lib.check(L.flgp_dev_u_recover(stages._st(), d_idx.data_ptr(), d_val.data_ptr(), n, r, dVs.data_ptr(), s, s, d_eig.data_ptr(), K,
                                    float(scale), 0, vectors.data_ptr(), n, None, work.data_ptr()))
    H = stages.hk(dev(values), t, vectors, dev(np.ascontiguousarray(V1.T)))
    stages.sync()
    return H.cpu().numpy().T


def check_both_ways(stages, case, dead=None):
    n, s, m, K, r = case
    idx, val, Vs, eig, values, V1 = inputs(n, s, m, K, r, dead)
    scale = math.sqrt(float(n))
    assert stages.L.flgp_dev_hk_rows_route(n, r, s, K, m) == 1
    H = run_hk_rows(stages, idx, val, Vs, eig, scale, values, T, V1)
    ref = R.hk_rows(idx, val, Vs, eig, scale, values, T, V1, w=device_weights(stages, values, T))
    assert np.array_equal(H, ref), "not the restatement's bits: %d of %d differ, max rel %.3e" % (
        np.count_nonzero(H != ref), H.size, np.abs(H - ref).max() / np.abs(ref).max())
    old = run_old_route(stages, idx, val, Vs, eig, scale, values, T, V1)
    err = np.abs(H - old).max() / np.abs(old).max()
    print("case", case, "vs u_recover + hk: max rel", err)
    assert err <= H_RTOL
    return H


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_bits_and_old_route(stages, knob, case):
    knob(2)                                      # wherever the row kernel applies: the rule is not what is tested here
    check_both_ways(stages, case)


def test_zero_eigenvalue_column_contributes_nothing(stages, knob):
    """eig_k = 0: q_k = 0, the column adds exact zeros to every chain -- H is the restatement's and, bit for bit, the H of
    the spectrum without that column"""
    knob(2)
    case = (10000, 5121, 5, 7, 10)
    H = check_both_ways(stages, case, dead=3)
    idx, val, Vs, eig, values, V1 = inputs(*case, 3)
    keep = [0, 1, 2, 4, 5, 6]
    H6 = run_hk_rows(stages, idx, val, Vs[:, keep], eig[keep], math.sqrt(1e4), values[keep], T, V1[:, keep])
    assert np.array_equal(H, H6)


def test_route_query(stages, knob):
    q = stages.L.flgp_dev_hk_rows_route
    knob(2)
    assert q(10000, 10, 5000, 200, 1000) == 1 and q(9999, 10, 5000, 200, 1000) == 0
    assert q(10000, 10, 20480, 200, 1000) == 1 and q(10000, 10, 20481, 200, 1000) == 0
    knob(1)                                      # the measured rule: K W / r >= 60 for m >= 480, >= 40 for 100 <= m < 480
    assert q(1_000_000, 10, 5000, 200, 1000) == 1 and q(9999, 10, 5000, 200, 1000) == 0
    assert q(1_000_000, 10, 5000, 100, 1000) == 0 and q(1_000_000, 10, 10000, 200, 1000) == 0
    assert q(1_000_000, 10, 5000, 150, 480) == 1 and q(1_000_000, 10, 5000, 149, 480) == 0
    assert q(1_000_000, 10, 5000, 100, 479) == 1 and q(1_000_000, 10, 5000, 99, 100) == 0
    assert q(1_000_000, 10, 10000, 200, 100) == 1 and q(1_000_000, 10, 5000, 200, 99) == 0
    assert q(1_000_000, 10, 20481, 200, 1000) == 0
    knob(0)
    assert q(1_000_000, 10, 5000, 200, 1000) == 0


def test_refused_where_no_slice_fits(stages):
    n, s, m, K, r = 9999, 64, 4, 7, 10
    idx, val, Vs, eig, values, V1 = inputs(n, s, m, K, r)
    L = stages.L
    H = stages.empty((m, n)); work = stages.empty((L.flgp_dev_hk_rows_workspace(s, m, K) // 8 + 1,))
    d = [dev(a) for a in (idx, val, np.ascontiguousarray(Vs.T), eig, values, np.ascontiguousarray(V1.T))]
    rc = L.flgp_dev_hk_rows(stages._st(), d[0].data_ptr(), d[1].data_ptr(), n, r, d[2].data_ptr(), s, s, d[3].data_ptr(), K, 1.0,
                            d[4].data_ptr(), T, d[5].data_ptr(), m, m, H.data_ptr(), n, work.data_ptr())
    assert rc != 0 and b"hk_rows" in L.flgp_last_error()


def sharded(stages, dX, dU, sizes, n, d, s, m, r, t, K, want_vectors):
    L = stages.L
    H = torch.full((m, n), float("nan"), dtype=torch.float64, device=DEV)
    vals = stages.empty((K,))
    vec = stages.empty((K, n)) if want_vectors else None
    _lib.check(L.flgp_dev_heat_kernel_covariance_sharded(stages._st(), None, dX.data_ptr(), n, n, d, n, 0, dU.data_ptr(), s, s,
                                                         sizes.data_ptr(), m, r, t, K, b"lae", b"cluster-normalized", 1, 0.1,
                                                         H.data_ptr(), n, vals.data_ptr(), vec.data_ptr() if want_vectors else None,
                                                         n, None))
    return H, vals, vec


def test_path_routes_agree(stages, knob):
    """The whole path through flgp_dev_heat_kernel_covariance_sharded at n = 12000, s = 600, K = 40, m = 64, the row route
    forced on (the rule says 0 here: m < 100).  With and without d_vectors_out -- the whole U-recovery, or the training rows
    alone -- H is the same bit for bit and so are the values; H is within 1e-8 max|H| of the knob-off path; and the
    knob-off H is, bit for bit, flgp_dev_hk on the vectors that call returns: the old route."""
    n, d, s, r, K, m, t = 12000, 3, 600, 5, 40, 64, 5.0
    X, U0, U = make_case(n, d, s, r, seed=9)
    dX = dev(np.ascontiguousarray(X.T)); dU = dev(np.ascontiguousarray(U0.T)); sizes = dev(U[:, d].copy())
    assert stages.L.flgp_dev_hk_rows_route(n, r, s, K, m) == 0
    knob(2)
    assert stages.L.flgp_dev_hk_rows_route(n, r, s, K, m) == 1
    Hv, vals_v, vec = sharded(stages, dX, dU, sizes, n, d, s, m, r, t, K, True)
    Hn, vals_n, _ = sharded(stages, dX, dU, sizes, n, d, s, m, r, t, K, False)
    assert torch.equal(Hv, Hn) and torch.equal(vals_v, vals_n)
    knob(0)
    Ho, vals_o, vec_o = sharded(stages, dX, dU, sizes, n, d, s, m, r, t, K, True)
    assert torch.equal(vals_o, vals_v) and torch.equal(vec_o, vec)
    err = float((Hv - Ho).abs().max() / Ho.abs().max())
    print("whole path, rows against MFMA route: max rel", err)
    assert err <= H_RTOL
    assert torch.equal(Ho, stages.hk(vals_o, t, vec_o, vec_o[:, :m].contiguous()))
