"""CPU: the numpy restatements of tests/np_sparse_stages.py against the compiled oracle, on the inputs that
tests/test_gpu_sparse_stages.py feeds the kernels.  What passes here is what gives the GPU module's bit-for-bit
assertions their meaning: the restatement is the oracle's arithmetic, and the inputs are ones on which another
summation order shows."""
import math

import numpy as np
import pytest

import np_sparse_stages as nps
from conftest import make_case

UR_IDS = [nps.u_recover_case_id(c) for c in nps.U_RECOVER_CASES]


def test_u_recover_cases_cover_every_route_and_edge():
    """the curated list holds what the issue of the GPU module asks of it, so that trimming it is noticed"""
    by = {}
    for route, K, n, r, s, root, scale, want_values, _ in nps.U_RECOVER_CASES:
        assert route == nps.u_recover_route(K, route != "null")
        by.setdefault(route, []).append((K, n, r, s, root, scale, want_values))
    want = dict(null=({1, 7, 8, 9, 65}, {1, 255, 256, 257}),
                tiled=({1, 63, 65, 129}, {1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 130}),
                kpl2=({2, 126, 130, 258}, {1, 63, 64, 65, 130}),
                kpl4=({4, 252, 256, 260, 516}, {1, 7, 8, 9, 31, 32, 33, 70}))
    tile = dict(null=(8, 256), tiled=(64, 64), kpl2=(128, 64), kpl4=(256, 32))
    for route, (Ks, ns) in want.items():
        rows = by[route]
        assert {c[0] for c in rows} == Ks and {c[1] for c in rows} == ns
        assert {c[2] for c in rows} == {1, 3, 10, 32} and {c[3] for c in rows} == {31, 32, 33, 97}
        assert {c[4] for c in rows} == {0, 1} and {c[5] for c in rows} == {"sqrtn", "third"}
        assert any(not c[6] for c in rows)
        kt, rt = tile[route]        # more than one column tile together with a ragged last row block
        assert any(c[0] > kt and c[1] > rt and c[1] % rt for c in rows)


@pytest.mark.parametrize("case", nps.U_RECOVER_CASES, ids=UR_IDS)
def test_u_recover_restatement_is_the_oracle(oracle, case):
    route, K, n, r, s, root, scale, want_values, seed = case
    idx, val, V, eig = nps.u_recover_inputs(K, n, r, s, seed)
    assert idx.min() >= 0 and idx.max() < s and 0 in idx[0] and s - 1 in idx[-1]
    assert (eig > 0).all() and (np.diff(eig) <= 0).all()
    assert (val > 0).any() and (val < 0).any() or val.size < 4
    out, values = nps.u_recover(idx, val, V, eig, math.sqrt(float(n)), root=bool(root))
    ref = oracle.u_recover(idx, val, s, V, np.sqrt(eig))
    np.testing.assert_array_equal(out, ref)                      # every sigma is positive here
    np.testing.assert_array_equal(values, np.sqrt(eig) if root else eig)


def test_u_recover_restatement_zero_sigma_rule(oracle):
    """an exact 0.0, a negative entry and -0.0: those columns are +0.0, the others the oracle's"""
    K, n, r, s = 9, 40, 10, 33
    idx, val, V, eig = nps.u_recover_inputs(K, n, r, s, 1)
    eig[[2, 5, 8]] = [0.0, -0.25, -0.0]
    for root in (False, True):
        out, values = nps.u_recover(idx, val, V, eig, math.sqrt(n), root=root)
        dead = np.array([2, 5, 8]); live = np.setdiff1d(np.arange(K), dead)
        assert (out[:, dead] == 0.0).all() and not np.signbit(out[:, dead]).any()
        assert (values[dead] == 0.0).all() and not np.signbit(values[dead]).any()
        with np.errstate(divide="ignore", invalid="ignore"):
            ref = oracle.u_recover(idx, val, s, V, np.sqrt(np.maximum(eig, 0.0)))
        np.testing.assert_array_equal(out[:, live], ref[:, live])


@pytest.mark.parametrize("case", [c for c in nps.U_RECOVER_CASES if c[3] >= 3],
                         ids=[nps.u_recover_case_id(c) for c in nps.U_RECOVER_CASES if c[3] >= 3])
def test_u_recover_inputs_expose_a_reordered_sum(case):
    """walking a in descending order changes at least one entry: the GPU module's bit-for-bit comparison can see a
    kernel that sums in another order"""
    route, K, n, r, s, root, scale, want_values, seed = case
    idx, val, V, eig = nps.u_recover_inputs(K, n, r, s, seed)
    sc = nps.u_recover_scale(scale, n)
    fwd, _ = nps.u_recover(idx, val, V, eig, sc)
    rev, _ = nps.u_recover(idx, val, V, eig, sc, descending=True)
    assert (fwd != rev).any()
    np.testing.assert_allclose(rev, fwd, rtol=0, atol=1e-12 * np.abs(fwd).max())    # the same sum all the same


# ------------------------------------------------------------------------------------------------------------ Laplacian
@pytest.mark.parametrize("n", [257, 700])
@pytest.mark.parametrize("r", [1, 10, 25, 32])
def test_two_pass_laplacian_is_the_oracle(oracle, n, r):
    d, s = 3, 48
    X, U0, U = make_case(n, d, s, r, seed=n + r)
    ei, zl = oracle.lae(X, U0, r)
    for gl in ("rw", "normalized", "cluster-normalized"):
        zn = nps.graph_laplacian(ei, zl, s, gl, U[:, d])
        np.testing.assert_array_equal(zn, oracle.graph_laplacian(ei, zl, s, gl, U[:, d]))
        oi, oz = oracle.cross_similarity(X, U, r, gl=gl)
        np.testing.assert_array_equal(oi, ei)
        np.testing.assert_array_equal(zn, oz)


@pytest.mark.parametrize("r", [1, 24, 25, 32])
def test_two_pass_laplacian_on_the_random_ell_inputs(oracle, r):
    n, s = 700, 48
    idx, val, sizes = nps.ell_inputs(n, s, r, seed=5)
    assert (np.diff(idx, axis=1) > 0).all() and idx.min() >= 0 and idx.max() < s and (val > 0).all()
    c = nps.colsum(idx, val, s)
    np.testing.assert_array_equal(c, oracle.colsum(idx, val, s))
    for gl, nc in (("rw", None), ("normalized", None), ("cluster-normalized", sizes)):
        np.testing.assert_array_equal(nps.graph_laplacian(idx, val, s, gl, nc), oracle.graph_laplacian(idx, val, s, gl, nc))
    av, oc = oracle.scale_A(idx, val, s)
    np.testing.assert_array_equal(nps.col_scale(idx, val, c, None, 1), av)


@pytest.mark.parametrize("n,s,r", [(700, 40, 17), (2049, 65, 32), (3000, 65, 16)])
def test_colsum_restatement_across_chunks(oracle, n, s, r):
    idx, val, _ = nps.ell_inputs(n, s, r, seed=9)
    np.testing.assert_array_equal(nps.colsum(idx, val, s), oracle.colsum(idx, val, s))


# ----------------------------------------------------------------------------------------------------------------- mean
@pytest.mark.parametrize("count", nps.MEAN_COUNTS)
def test_mean_restatement_within_the_summation_bound(count):
    """count - 1 rounded additions of partial sums no larger than count max|x|, and one rounded division: an error of
    at most count 2^-53 max|x| whatever the tree.  A bound from the arithmetic, not a measurement."""
    x = nps.mean_inputs(count)
    assert count < 4000 or np.abs(x).max() > 1e12 * np.abs(x).min()
    got = nps.mean(x)
    assert abs(got - math.fsum(x) / count) <= count * 2.0 ** -53 * np.abs(x).max()


def test_mean_restatement_follows_the_tree():
    """values the tree adds exactly, placed so that a strictly sequential sum would lose them"""
    x = np.zeros(4096 + 300)
    x[0] = 1.0; x[256] = 2.0 ** -53; x[512] = 2.0 ** -53      # lane 0: (1 + 2^-53) + 2^-53 = 1 (each add rounds to even)
    x[1] = 2.0 ** -53; x[257] = 2.0 ** -53                    # lane 1: 2^-52, then 1 + 2^-52 in the last halving step
    x[4096 + 299] = 2.0 ** -52                                # second slab, added to the first slab's total
    assert nps.mean(x) == (1.0 + 2.0 ** -51) / x.size
    acc = 0.0
    for v in x:
        acc = acc + v
    assert acc == 1.0 + 2.0 ** -52                            # (what the strictly sequential order gives instead)
