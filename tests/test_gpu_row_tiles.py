"""GPU (-m gpu): the wave tiles of the ELL rows (csrc/sparse.hip: flgp_dev_row_tiles_pack) and the two entries that read them,
flgp_dev_u_recover_tiles and flgp_dev_hk_rows_tiles.

The pack is held, byte for byte, to the numpy restatement of the layout (tests/np_row_tiles.py) with NaN on both sides of the
buffer.  The tiles entries are held, bit for bit and over the whole output buffer (NaN guard rows and columns included),
to flgp_dev_u_recover / flgp_dev_hk_rows on the same inputs: only the loads differ, so nothing may.  Inputs as in
tests/test_gpu_hk_rows.py (val = normal x 10**uniform(-3, 3)), so that another order of a sum changes bits.

Shapes: n = 10000 (the smallest the LDS route takes; not a multiple of 64), 10048 (a multiple), 10001; r = 1, 3, 10, 11, 13,
25, 32 (one, two and three steps, odd r, n r odd); s = 5120, 5121, 6827, 10241 (W = 4, 3, 2, 1); K = 1, 7, 200 and
m = 5, 8, 1001 (off a multiple of W, several slices); ldo / ldh larger than n."""
import functools
import math

import numpy as np
import pytest
import torch

import np_row_tiles as T
from conftest import make_case
from flgp_amd import _lib
from flgp_amd.pipeline import HipStages

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = [10000, 10048, 10001]
RS = [1, 3, 10, 11, 13, 25, 32]

#           n      s      r   K
U_CASES = [
    (10000, 5120, 10, 200),
    (10001, 5121, 3, 7),
    (10000, 6827, 11, 1),
    (10048, 10241, 13, 7),
    (10001, 5120, 25, 7),
    (10000, 5121, 32, 200),
    (10001, 6827, 1, 7),
    (10000, 10241, 10, 1),
    (10048, 5120, 13, 1),
]
#           n      s      r   K   m
H_CASES = [
    (10000, 5120, 10, 7, 1001),
    (10001, 5121, 3, 7, 5),
    (10000, 6827, 11, 1, 8),
    (10048, 10241, 13, 7, 5),
    (10001, 5120, 25, 7, 8),
    (10000, 5121, 32, 7, 1001),
    (10001, 6827, 1, 200, 5),
    (10000, 10241, 10, 7, 8),
    (10048, 5120, 13, 200, 5),
]


def test_the_cases_take_every_width_and_edge():
    for cases in (U_CASES, H_CASES):
        assert {c[0] for c in cases} == set(NS) and {c[2] for c in cases} == set(RS)
        assert {c[1] for c in cases} == {5120, 5121, 6827, 10241} and {c[3] for c in cases} == {1, 7, 200}
    assert {c[4] for c in H_CASES} == {5, 8, 1001}


@pytest.fixture(scope="module")
def stages():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    return HipStages(DEV)


@pytest.fixture()
def knobs(stages):
    """sets a knob and puts the defaults back"""
    def set_(key, v):
        stages.L.flgp_set_tuning(key, v)
    yield set_
    stages.L.flgp_set_tuning(b"hk_rows", 1)
    stages.L.flgp_set_tuning(b"row_tiles", 1)


@functools.lru_cache(maxsize=None)
def rows(n, s, r):
    """(idx, val) -- read-only, shared; indices over the whole of [0, s), first and last among them"""
    rng = np.random.default_rng([n, s, r])
    idx = rng.integers(0, s, size=(n, r)).astype(np.int32)
    idx[0, 0] = 0; idx[n - 1, r - 1] = s - 1
    val = rng.normal(size=(n, r)) * 10.0 ** rng.uniform(-3.0, 3.0, size=(n, r))
    idx.setflags(write=False); val.setflags(write=False)
    return idx, val


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def same_bits(a, b):
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


def packed(stages, d_idx, d_val, guard=16):
    """(tiles, whole buffer): the tile image inside `guard` NaN doubles on either side, on a 128-byte edge"""
    n, r = d_idx.shape
    nbytes = stages.L.flgp_dev_row_tiles_bytes(n, r)
    assert nbytes == T.image_bytes(n, r)
    buf = torch.full((nbytes // 8 + 2 * guard,), float("nan"), dtype=torch.float64, device=DEV)
    tiles = buf[guard:guard + nbytes // 8]
    assert tiles.data_ptr() % 128 == 0
    _lib.check(stages.L.flgp_dev_row_tiles_pack(stages._st(), d_idx.data_ptr(), d_val.data_ptr(), n, r, tiles.data_ptr()))
    stages.sync()
    return tiles, buf


@pytest.mark.parametrize("r", RS)
@pytest.mark.parametrize("n", NS)
def test_pack_is_the_restatement(stages, n, r):
    idx, val = rows(n, 5000, r)
    tiles, buf = packed(stages, dev(idx), dev(val))
    host = buf.cpu().numpy()
    assert np.isnan(host[:16]).all() and np.isnan(host[-16:]).all(), "written outside flgp_dev_row_tiles_bytes"
    image = host[16:-16].view(np.uint8)
    ref = T.pack(idx, val)
    assert image.size == ref.size and np.array_equal(image, ref)


def u_recover_both(stages, n, s, r, K):
    L = stages.L
    idx, val = rows(n, s, r)
    rng = np.random.default_rng([n, s, r, K, 1])
    V = rng.normal(size=(K, s))
    eig = np.sort(rng.uniform(0.05, 1.0, size=K))[::-1].copy()
    d_idx, d_val, dV, d_eig = dev(idx), dev(val), dev(V), dev(eig)
    tiles, _ = packed(stages, d_idx, d_val)
    ldo, scale = n + 5, math.sqrt(float(n))
    assert L.flgp_dev_u_recover_route(n, r, s, K, 1) == 4
    out = []
    for use_tiles in (False, True):
        vec = torch.full((K + 1, ldo), float("nan"), dtype=torch.float64, device=DEV)
        values = torch.full((K + 1,), float("nan"), dtype=torch.float64, device=DEV)
        work = stages.empty((L.flgp_dev_u_recover_workspace(s, K) // 8 + 1,))
        if use_tiles:
            rc = L.flgp_dev_u_recover_tiles(stages._st(), tiles.data_ptr(), n, r, dV.data_ptr(), s, s, d_eig.data_ptr(), K, scale, 1,
                                            vec.data_ptr(), ldo, values.data_ptr(), work.data_ptr())
        else:
            rc = L.flgp_dev_u_recover(stages._st(), d_idx.data_ptr(), d_val.data_ptr(), n, r, dV.data_ptr(), s, s, d_eig.data_ptr(), K,
                                      scale, 1, vec.data_ptr(), ldo, values.data_ptr(), work.data_ptr())
        stages.sync()
        assert rc == 0, L.flgp_last_error()
        out.append((vec, values))
    return out


@pytest.mark.parametrize("case", U_CASES, ids=["n%d-s%d-r%d-K%d" % c for c in U_CASES])
def test_u_recover_tiles_bits(stages, case):
    n, s, r, K = case
    (vec, values), (vec_t, values_t) = u_recover_both(stages, n, s, r, K)
    assert not torch.isnan(vec[:K, :n]).any() and torch.isnan(vec[K]).all() and torch.isnan(vec[:K, n:]).all()
    assert same_bits(vec, vec_t) and same_bits(values, values_t)


def hk_rows_both(stages, n, s, r, K, m):
    L = stages.L
    idx, val = rows(n, s, r)
    rng = np.random.default_rng([n, s, r, K, m])
    Vs = rng.normal(size=(K, s)); V1 = rng.normal(size=(K, m))
    eig = np.sort(rng.uniform(0.05, 1.0, size=K))[::-1].copy()
    d_idx, d_val, dVs, dV1, d_eig, d_values = dev(idx), dev(val), dev(Vs), dev(V1), dev(eig), dev(np.sqrt(eig))
    tiles, _ = packed(stages, d_idx, d_val)
    ldh, scale = n + 5, math.sqrt(float(n))
    out = []
    for use_tiles in (False, True):
        H = torch.full((m + 1, ldh), float("nan"), dtype=torch.float64, device=DEV)
        work = stages.empty((L.flgp_dev_hk_rows_workspace(s, m, K) // 8 + 1,))
        if use_tiles:
            rc = L.flgp_dev_hk_rows_tiles(stages._st(), tiles.data_ptr(), n, r, dVs.data_ptr(), s, s, d_eig.data_ptr(), K, scale,
                                          d_values.data_ptr(), 10.0, dV1.data_ptr(), m, m, H.data_ptr(), ldh, work.data_ptr())
        else:
            rc = L.flgp_dev_hk_rows(stages._st(), d_idx.data_ptr(), d_val.data_ptr(), n, r, dVs.data_ptr(), s, s, d_eig.data_ptr(), K,
                                    scale, d_values.data_ptr(), 10.0, dV1.data_ptr(), m, m, H.data_ptr(), ldh, work.data_ptr())
        stages.sync()
        assert rc == 0, L.flgp_last_error()
        out.append(H)
    return out


@pytest.mark.parametrize("case", H_CASES, ids=["n%d-s%d-r%d-K%d-m%d" % c for c in H_CASES])
def test_hk_rows_tiles_bits(stages, case):
    n, s, r, K, m = case
    H, H_t = hk_rows_both(stages, n, s, r, K, m)
    assert not torch.isnan(H[:m, :n]).any() and torch.isnan(H[m]).all() and torch.isnan(H[:m, n:]).all()
    assert same_bits(H, H_t)


@pytest.mark.parametrize("n,s", [(9999, 64), (10000, 20481)])
def test_refused_where_the_routes_refuse(stages, knobs, n, s):
    L = stages.L
    r, K, m = 10, 7, 4
    knobs(b"hk_rows", 2)
    assert L.flgp_dev_u_recover_route(n, r, s, K, 1) != 4 and L.flgp_dev_hk_rows_route(n, r, s, K, m) == 0
    assert L.flgp_dev_row_tiles_route(n, r, s) == 0
    idx, val = rows(n, s, r)
    tiles, _ = packed(stages, dev(idx), dev(val))
    rng = np.random.default_rng(3)
    dV, dV1 = dev(rng.normal(size=(K, s))), dev(rng.normal(size=(K, m)))
    d_eig = dev(np.linspace(1.0, 0.1, K)); d_values = d_eig.sqrt()
    vec = stages.empty((K, n)); H = stages.empty((m, n))
    work = stages.empty((L.flgp_dev_u_recover_workspace(s, K) // 8 + 1,))
    rc = L.flgp_dev_u_recover_tiles(stages._st(), tiles.data_ptr(), n, r, dV.data_ptr(), s, s, d_eig.data_ptr(), K, 1.0, 1,
                                    vec.data_ptr(), n, None, work.data_ptr())
    assert rc != 0 and b"u_recover_tiles" in L.flgp_last_error()
    work = stages.empty((L.flgp_dev_hk_rows_workspace(s, m, K) // 8 + 1,))
    rc = L.flgp_dev_hk_rows_tiles(stages._st(), tiles.data_ptr(), n, r, dV.data_ptr(), s, s, d_eig.data_ptr(), K, 1.0,
                                  d_values.data_ptr(), 10.0, dV1.data_ptr(), m, m, H.data_ptr(), n, work.data_ptr())
    assert rc != 0 and b"hk_rows_tiles" in L.flgp_last_error()
    stages.sync()


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


def test_whole_path_with_and_without_tiles(stages, knobs):
    """flgp_dev_heat_kernel_covariance_sharded at n = 12000, d = 3, s = 600, r = 5, K = 40, m = 64 with the row route forced
    on: H, values and vectors are the same bits with row_tiles 0 and 1, with the vectors asked for (the whole U-recovery
    reads the tiles) and without (the training rows alone are recovered, the tiles serve the heat-kernel rows)."""
    n, d, s, r, K, m, t = 12000, 3, 600, 5, 40, 64, 5.0
    X, U0, U = make_case(n, d, s, r, seed=9)
    dX = dev(np.ascontiguousarray(X.T)); dU = dev(np.ascontiguousarray(U0.T)); sizes = dev(U[:, d].copy())
    knobs(b"hk_rows", 2)
    assert stages.L.flgp_dev_hk_rows_route(n, r, s, K, m) == 1
    got = {}
    for tiles in (0, 1):
        knobs(b"row_tiles", tiles)
        assert stages.L.flgp_dev_row_tiles_route(n, r, s) == tiles
        got[tiles] = [sharded(stages, dX, dU, sizes, n, d, s, m, r, t, K, want) for want in (True, False)]
    for (H0, vals0, vec0), (H1, vals1, vec1) in zip(got[0], got[1]):
        assert not torch.isnan(H1).any()
        assert torch.equal(H0, H1) and torch.equal(vals0, vals1)
        assert (vec0 is None and vec1 is None) or torch.equal(vec0, vec1)


def test_python_path_with_and_without_tiles(stages, knobs):
    """the Python driver (HeatKernelPath.run) at the same shape: the same bits with row_tiles 0 and 1"""
    from flgp_amd.pipeline import HeatKernelPath, PathConfig
    n, d, s, r, K, m, t = 12000, 3, 600, 5, 40, 64, 5.0
    X, U0, U = make_case(n, d, s, r, seed=9)
    dX = dev(np.ascontiguousarray(X.T)); dU = dev(np.ascontiguousarray(U0.T)); sizes = dev(U[:, d].copy())
    path = HeatKernelPath(stages)
    cfg = PathConfig(s=s, r=r, K=K, t=t, m=m)
    knobs(b"hk_rows", 2)
    got = {}
    for tiles in (0, 1):
        knobs(b"row_tiles", tiles)
        got[tiles] = path.run(dX, dU, cfg, n, 0, num_class=sizes)
        stages.sync()
    assert not torch.isnan(got[1].H).any()
    assert torch.equal(got[0].H, got[1].H) and torch.equal(got[0].vectors, got[1].vectors)
    assert torch.equal(got[0].values, got[1].values)
