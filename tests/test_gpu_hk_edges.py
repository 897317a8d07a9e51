"""GPU: the two LDS-panel kernels of flgp_dev_hk -- hk_panel2_kernel (csrc/hk2.hip) and hk_panel_kernel (csrc/hk.hip) -- at
their panel, tile and K edges, on shapes of a few hundred rows: the tuning keys hk_panel_min_n0 / hk_panel_min_n1 /
hk_panel2_min_n1 let the kernels take them and hk_panel_grid caps the grid, so that one workgroup walks several panels
(hk2: both LDS copies of the A part in turn, the next panel's A part through the register chunk during the last tile, its B
part through fetch_B / put_B, the next panel clamped to the last one; hk: the prefetch at pf_at, at stage 0, and by waves
without a stage).  hk_cases.py holds the tables and restates what each case reaches; test_hk_case_table.py (CPU) asserts it.

Every call goes straight to flgp_dev_hk.  Every operand is a column-major block at a row offset inside NaN (rows before and
behind it, the columns k >= K): a kernel that multiplies padding by zero where it should select it away gives NaN.  H lies
inside canaries with ldh > n0; every element inside must have been written, every canary must be intact.  The workspace
belongs to the test: NaN, exactly flgp_dev_hk_workspace bytes, and behind it a guard of canaries as long again that must be
intact -- a kernel that writes past the workspace fails here instead of damaging somebody else's memory.

Exact references.  Integers: V0 and V1 hold integers from [-8, 8] and lambda = 1, so every weight is exp(-0) = 1 (asserted
on the device once), every product an integer of magnitude <= 64 and every partial sum one of magnitude <= 64 * 288 -- exact
in any order, compared with assert_array_equal against numpy's V0 @ V1.T.  Weight mapping: distinct lambda, V1's rows one-hot
at k_b, so H(a, b) = V0(a, k_b) w[k_b] with one rounding (the other terms of the chain are exact zeros); w is the device's
own (its exp may differ from numpy's in the last bit), read through the GEMM route."""
import contextlib
import functools
import zlib

import numpy as np
import pytest
import torch

import hk_cases as C
from flgp_amd import _lib, api
from flgp_amd.pipeline import HipStages

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 1.7
LONGDOUBLE_OK = np.finfo(np.longdouble).nmant >= 63


@pytest.fixture(scope="module")
def stages():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    return HipStages(DEV)


@contextlib.contextmanager
def tuned(L, **keys):
    try:
        for k, v in keys.items():
            L.flgp_set_tuning(k.encode(), v)
        yield
    finally:
        for k, v in C.DEFAULTS.items():
            L.flgp_set_tuning(k.encode(), v)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def ints(rng, shape):
    return rng.integers(-8, 9, size=shape).astype(np.float64)


def case_rng(cs, what):
    return np.random.default_rng(zlib.crc32((C.case_id(cs) + what).encode()))


@functools.lru_cache(maxsize=None)
def distinct_values(K):
    v = np.sort(np.random.default_rng(K).uniform(0.05, 1.0, size=K))[::-1].copy()
    assert np.unique(v).size == K
    v.setflags(write=False)
    return v


_weights = {}


def device_weights(stages, K):
    """w_k = exp(-t (1 - lambda_k)) as the device computes it, read through the small GEMM route (nothing tuned) on identity
    blocks: H = I diag(w) I^T is exact.  Held to numpy's within two units in the last place."""
    if K not in _weights:
        values = distinct_values(K)
        assert stages.L.flgp_dev_hk_route(K, K, K, K) == 0
        eye = torch.eye(K, dtype=torch.float64, device=DEV)
        w = torch.diagonal(stages.hk(dev(values), T, eye, eye)).cpu().numpy().copy()
        wn = np.exp(-T * (1.0 - values))
        assert (np.abs(w - wn) <= 2.0 * np.spacing(wn)).all()
        _weights[K] = w
    return _weights[K]


def test_unit_eigenvalues_give_unit_weights(stages):
    """lambda = 1: the weight is exp(-t * 0) = 1 exactly -- what makes the integer reference exact"""
    K = 288
    eye = torch.eye(K, dtype=torch.float64, device=DEV)
    w = torch.diagonal(stages.hk(torch.ones(K, dtype=torch.float64, device=DEV), T, eye, eye)).cpu().numpy()
    np.testing.assert_array_equal(w, np.ones(K))


class Operand:
    """A logical operand (n x K) taken from a source placed on the device: a range of its rows, or a gather"""

    def __init__(self, logical, mode, rng):
        n, K = logical.shape
        rows, idx, ns = C.rows_of(mode, n, rng)
        src = np.full((ns, K), np.nan)              # source rows no index names: NaN
        src[rows] = logical
        self.logical = src[rows]                    # (a repeated row: the later write won)
        self.placed = C.place(src, device=DEV)
        self.d_idx = None if idx is None else dev((idx + self.placed.off).astype(np.int32))
        self.row0 = self.placed.off if idx is None else 0

    @property
    def idx_ptr(self):
        return None if self.d_idx is None else self.d_idx.data_ptr()


def call_hk(L, values, op0, op1, K):
    """flgp_dev_hk on two operands; returns H (n0 x n1) after checking the return code, that every element of H was written,
    the canaries around H and the guard behind the workspace"""
    n0, n1 = op0.logical.shape[0], op1.logical.shape[0]
    gather0 = op0.d_idx is not None
    wb = L.flgp_dev_hk_workspace(n0, n1, K, int(gather0))
    assert wb % 8 == 0
    nw = wb // 8
    host = np.full(2 * nw + 64, np.nan)
    host[nw:].view(np.int64)[:] = C.CANARY_BITS
    work = torch.from_numpy(host).to(DEV)
    H = C.place_result(n0, n1, device=DEV)
    d_values = dev(values)
    rc = L.flgp_dev_hk(torch.cuda.current_stream().cuda_stream, d_values.data_ptr(), K, T, op0.placed.ptr, op0.placed.ld,
                       op0.idx_ptr, op0.row0, n0, op1.placed.ptr, op1.placed.ld, op1.idx_ptr, op1.row0, n1, H.ptr, H.ldh,
                       work.data_ptr())
    torch.cuda.synchronize()
    _lib.check(rc)
    guard = work[nw:].cpu().numpy().view(np.int64)
    assert (guard == C.CANARY_BITS).all(), "a write behind the workspace: %d of the guard's doubles changed, the first %d past its end" % (
        np.count_nonzero(guard != C.CANARY_BITS), int(np.flatnonzero(guard != C.CANARY_BITS)[0]))
    got, written, outside_ok = H.read()
    assert outside_ok, "a store outside H"
    assert written, "%d elements of H were not written" % np.count_nonzero(got.view(np.int64) == C.CANARY_BITS)
    return got


def check_route(L, cs, want, ldh=None):
    n0, n1, K = cs["n0"], cs["n1"], cs["K"]
    ldh = n0 + 5 if ldh is None else ldh
    got = L.flgp_dev_hk_route(n0, n1, K, ldh)
    assert got == want, "flgp_dev_hk_route(%d, %d, %d, %d) = %d, the restatement says %d" % (n0, n1, K, ldh, got, want)


def first_difference(got, ref):
    bad = np.argwhere(~(got == ref))
    a, b = bad[0]
    return "%d of %d elements differ, the first at (%d, %d): %r != %r" % (len(bad), ref.size, a, b, got[a, b], ref[a, b])


# ------------------------------------------------------------------------------------------------- the three checks of a case
def exact_integers(L, cs, want_route, tune=None):
    n0, n1, K = cs["n0"], cs["n1"], cs["K"]
    rng = case_rng(cs, "ints")
    op0 = Operand(ints(rng, (n0, K)), "gather" if cs["gather0"] else "range", rng)
    op1 = Operand(ints(rng, (n1, K)), cs["idx1"], rng)
    with tuned(L, **(C.case_tuning(cs) if tune is None else tune)):
        check_route(L, cs, want_route)
        H = call_hk(L, np.ones(K), op0, op1, K)
    ref = op0.logical @ op1.logical.T
    same = np.array_equal(H, ref)
    assert same, first_difference(H, ref)


def weight_mapping(stages, cs, want_route):
    L = stages.L
    n0, n1, K = cs["n0"], cs["n1"], cs["K"]
    values, w = distinct_values(K), device_weights(stages, K)
    rng = case_rng(cs, "one-hot")
    op0 = Operand(ints(rng, (n0, K)), "gather" if cs["gather0"] else "range", rng)
    step = n1 - 1 if (cs["idx1"] == "repeat" and n1 >= 2) else n1        # (a repeated row shows its k twice)
    seen = set()
    with tuned(L, **C.case_tuning(cs)):
        check_route(L, cs, want_route)
        for rnd in range(C.ceil_div(K, step)):
            kb = (np.arange(n1) + rnd * step) % K
            op1 = Operand(np.eye(K)[kb], cs["idx1"], rng)
            kb = np.argmax(op1.logical, axis=1)
            assert (op1.logical.sum(axis=1) == 1.0).all()
            seen |= set(kb.tolist())
            H = call_hk(L, values, op0, op1, K)
            ref = op0.logical[:, kb] * w[kb][None, :]
            same = np.array_equal(H, ref)
            assert same, "round %d: %s" % (rnd, first_difference(H, ref))
    assert seen == set(range(K)), "the one-hot rows did not reach every k"


def routes_agree(L, cs, routes):
    """N(0, 1) data: H of every route the case can take, bit for bit the tiled GEMM's"""
    n0, n1, K = cs["n0"], cs["n1"], cs["K"]
    rng = case_rng(cs, "normal")
    op0 = Operand(rng.normal(size=(n0, K)), "gather" if cs["gather0"] else "range", rng)
    op1 = Operand(rng.normal(size=(n1, K)), cs["idx1"], rng)
    values = distinct_values(K)
    out = {}
    for r in routes:
        off = {2: {}, 1: {"hk_panel2": 0}, 0: {"hk_panel": 0}}[r]
        with tuned(L, **dict(C.case_tuning(cs), **off)):
            check_route(L, cs, r)
            out[r] = call_hk(L, values, op0, op1, K)
    assert not np.isnan(out[0]).any()
    for r in routes[:-1]:
        same = np.array_equal(out[r].view(np.int64), out[0].view(np.int64))
        assert same, "route %d against the GEMM: %s" % (r, first_difference(out[r].view(np.int64), out[0].view(np.int64)))


# ------------------------------------------------------------------------------------------------- hk_panel2_kernel
HK2_IDS = [C.case_id(c) for c in C.HK2_CASES]


@pytest.mark.parametrize("cs", C.HK2_CASES, ids=HK2_IDS)
def test_hk2_exact_on_integers(stages, cs):
    exact_integers(stages.L, cs, 2)


@pytest.mark.parametrize("cs", C.HK2_CASES, ids=HK2_IDS)
def test_hk2_weight_mapping(stages, cs):
    """pins the swizzle of hk2_scale_kernel and the k of every weight: column b of H is column k_b of V0 times w[k_b]"""
    weight_mapping(stages, cs, 2)


@pytest.mark.parametrize("cs", C.HK2_CASES, ids=HK2_IDS)
def test_hk2_routes_agree(stages, cs):
    routes_agree(stages.L, cs, (2, 1, 0))


# ------------------------------------------------------------------------------------------------- hk_panel_kernel
HK_IDS = [C.case_id(c) for c in C.HK_CASES]


@pytest.mark.parametrize("cs", C.HK_CASES, ids=HK_IDS)
def test_hk_exact_on_integers(stages, cs):
    exact_integers(stages.L, cs, 1)


@pytest.mark.parametrize("cs", C.HK_CASES, ids=HK_IDS)
def test_hk_weight_mapping(stages, cs):
    weight_mapping(stages, cs, 1)


@pytest.mark.parametrize("cs", C.HK_CASES, ids=HK_IDS)
def test_hk_routes_agree(stages, cs):
    routes_agree(stages.L, cs, (1, 0))


@pytest.mark.parametrize("cs", C.HK2_CASES, ids=HK2_IDS)
def test_hk_exact_on_integers_at_the_hk2_cases(stages, cs):
    """hk_panel_kernel at the shapes and K of the other table (hk_panel2 = 0): the stage counts 6, 7, 12 and 13 in between, and
    waves with two to five m-tiles"""
    exact_integers(stages.L, cs, 1, dict(C.case_tuning(cs), hk_panel2=0))


# ------------------------------------------------------------------------------------------------- the route's K boundaries
@pytest.mark.parametrize("cs", C.ROUTE_CASES, ids=[C.case_id(c) for c in C.ROUTE_CASES])
def test_route_boundaries(stages, cs):
    """K = 88 | 89, 112 | 113, 184 | 185, 208 | 209: hk_panel_kernel next to every hk_panel2_kernel instance; 288 | 289: the
    GEMM beyond eighteen stages.  Exact on integers on whichever route it is."""
    exact_integers(stages.L, cs, C.route(cs["n0"], cs["n1"], cs["K"], cs["n0"] + 5, C.case_tuning(cs)))


# ------------------------------------------------------------------------------------------------- rounding
@pytest.mark.skipif(not LONGDOUBLE_OK, reason="np.longdouble has fewer than 63 mantissa bits here: no reference finer than float64")
@pytest.mark.parametrize("cs,kernel", [(C.ROUNDING_HK2, 2), (C.ROUNDING_HK, 1)], ids=["hk2", "hk"])
def test_rounding_on_normal_data(stages, cs, kernel):
    """N(0, 1) data against np.longdouble.  The bound is the elementwise (K + 2) 2^-53 (|V0| |V1 o w|^T) with the device's
    own w: K roundings of the multiply-add chain, one for V1 w, one more to absorb the second order -- derived, not measured."""
    L = stages.L
    n0, n1, K = cs["n0"], cs["n1"], cs["K"]
    values, w = distinct_values(K), device_weights(stages, K)
    rng = case_rng(cs, "rounding")
    op0 = Operand(rng.normal(size=(n0, K)), "gather" if cs["gather0"] else "range", rng)
    op1 = Operand(rng.normal(size=(n1, K)), cs["idx1"], rng)
    with tuned(L, **C.case_tuning(cs)):
        check_route(L, cs, kernel)
        H = call_hk(L, values, op0, op1, K)
    ld = np.longdouble
    Vw = op1.logical.astype(ld) * w.astype(ld)[None, :]
    ref = op0.logical.astype(ld) @ Vw.T
    bound = ld(K + 2) * ld(2.0) ** -53 * (np.abs(op0.logical).astype(ld) @ np.abs(Vw).T)
    err = np.abs(H.astype(ld) - ref)
    print("%s: max err / bound = %.3f" % (C.case_id(cs), float((err / bound).max())))
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------- the shipped launch configuration
@pytest.mark.parametrize("n1,K,kernel", [(480, 100, 2), (64, 40, 1)], ids=["hk2", "hk"])
def test_uncapped_grid_walks_panels(stages, n1, K, kernel):
    """nothing tuned: one workgroup per CU, two panels for each and a ragged third for three of them"""
    L = stages.L
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n0 = 64 * (2 * cus + 3) - 27
    cs = C.case(n0, 0, n1, K)
    f = C.panel_facts(n0, cus)
    assert f["grid"] == cus and sorted(set(f["per_wg"])) == [2, 3] and f["ragged_by_prefetch"]
    assert C.route(n0, n1, K, n0 + 5) == kernel
    exact_integers(L, cs, kernel, {})


# ------------------------------------------------------------------------------------------------- through the host entry
def test_host_entry_with_gathered_rows_where_the_operand_was_short(stages):
    """HK_from_spectrum_cpp, gathered idx0, K = 190: the gathered rows of V0 lie right behind the small operand in the
    workspace, whose hk2 layout (208 columns) was longer than the 192 it was sized for -- the head of the gathered block
    was overwritten and H silently wrong.  Integers, lambda = 1: exact."""
    n0, n1, K, n = 2100, 480, 190, 2150
    assert stages.L.flgp_dev_hk_route(n0, n1, K, n0) == 2
    rng = np.random.default_rng(190)
    vec = np.asfortranarray(ints(rng, (n, K)))
    ep = api.EigenPair(np.ones(K), vec)
    idx0 = rng.permutation(n)[:n0].astype(np.int32)
    idx1 = np.arange(3, 3 + n1, dtype=np.int32)
    H = api.HK_from_spectrum_cpp(ep, K, T, idx0, idx1)
    ref = vec[idx0] @ vec[idx1].T
    same = np.array_equal(H, ref)
    assert same, first_difference(H, ref)
