"""GPU: the one-vs-rest logit posterior in one call (flgp_eigenpair_logit_posterior_multiclass and its _nll
variant).  The contract is bit for bit: column j of mean / cov and iters[j] are the bytes of the binary entry
flgp_eigenpair_logit_posterior on Y == j at ts[j], on both sides of m = K, for ranges and index sets, every J and every
chunk size (max_parallel); nll is the bytes of negative_log_likelihood on the returned arrays.  One independent anchor against
the dense numpy restatement (tests/np_logit_posterior.py) under its existing tolerances, and the refusals.

Both entries run one body in the library (the binary entry is its batch of one), so the comparisons with the binary entry
here are consistency checks; the independent reference is the pinned bits of the loops the entries ran before
(tests/golden/logit_posterior_bits.npz, test_gpu_logit_posterior_bits.py).

The pair is tests/test_gpu_logit_posterior.py's (3000 rows, 200 columns, seed 101); ts[j] = 0.5 + 0.7 j."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

from flgp_amd import _lib, api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_logit_posterior as ref  # noqa: E402

pytestmark = pytest.mark.gpu

N = 3000
SIGMAS = [(0.0, 1e-3), (1e-3, 1e-3), (0.1, 0.0)]      # sigma11, sigma22
KS = [1, 15, 16, 17, 63, 64, 65, 120, 121, 129, 200]


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()


@functools.lru_cache(maxsize=None)
def host_pair(n, K, seed):
    """tests/test_gpu_logit_posterior.py::host_pair"""
    rng = np.random.default_rng(seed)
    values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
    return values, np.asfortranarray(rng.standard_normal((n, K)))


def resident(n, K, seed):
    values, V = host_pair(n, K, seed)
    return values, V, api.ResidentEigenPair.from_host(api.EigenPair(values, V))


@pytest.fixture(scope="module")
def pair():
    values, V, rp = resident(N, 200, 101)
    yield values, V, rp
    rp.free()


def ts_of(J):
    return 0.5 + 0.7 * np.arange(J)


def problem(m, mnew, J, kind, seed, n=N, empty=None):
    """idx0, idx1, labels: idx1 a range, or a permuted index set that shares rows with idx0; `empty`: a class without a member."""
    rng = np.random.default_rng(seed)
    if kind == "range":
        start = int(rng.integers(0, n - mnew - m + 1))
        idx0 = np.arange(start, start + m); idx1 = np.arange(n - mnew, n)
    else:
        perm = rng.permutation(n)
        idx0 = perm[:m]
        shared = min(m, mnew // 3)
        idx1 = rng.permutation(np.r_[idx0[:shared], perm[m:m + mnew - shared]])
    Y = rng.integers(0, J, m).astype(np.float64)
    if empty is not None:
        Y[Y == empty] = empty + 1
    return idx0, idx1, Y


def binary_columns(rp, idx0, idx1, K, ts, Y, s11, s22, **kw):
    """What a caller does without the entry: J calls of the binary entry, stacked."""
    J = len(ts)
    mean = np.zeros((len(idx1), J), order="F"); cov = np.zeros((len(idx1), J), order="F"); its = np.zeros(J, dtype=np.int32)
    for j in range(J):
        post, its[j] = rp.logit_posterior(idx0, idx1, K, ts[j], (Y == j).astype(np.float64), s11, s22, return_iters=True, **kw)
        mean[:, j] = post["mean"]; cov[:, j] = post["cov"]
    return mean, cov, its


def assert_same_bytes(got, its, mean, cov, its_ref, what):
    assert got["mean"].shape == mean.shape and got["mean"].flags.f_contiguous and got["cov"].flags.f_contiguous, what
    for j in range(mean.shape[1]):
        assert got["mean"][:, j].tobytes() == mean[:, j].tobytes(), f"{what}: mean, class {j}"
        assert got["cov"][:, j].tobytes() == cov[:, j].tobytes(), f"{what}: cov, class {j}"
    assert np.array_equal(its, its_ref), (what, its, its_ref)


def compare(rp, K, m, mnew, J, kind, sig, seed, empty=None, n=N, **kw):
    s11, s22 = sig
    idx0, idx1, Y = problem(m, mnew, J, kind, seed, n=n, empty=empty)
    ts = ts_of(J)
    mean, cov, its_ref = binary_columns(rp, idx0, idx1, K, ts, Y, s11, s22)
    got, its = rp.logit_posterior_multiclass(idx0, idx1, K, ts, Y, s22, sigma11=s11, return_iters=True, **kw)
    assert_same_bytes(got, its, mean, cov, its_ref, f"K={K} m={m} m_new={mnew} J={J} {kind} sigma={sig}")
    return its


# ---- 1. bit for bit against the binary entry, m > K ----------------------------------------------------------------------
# every K with J = 10 and m_new = 300 at its three m; the row-set kind and the sigmas go round with the case number
BIG = [(K, m, ("range", "perm")[(a + b) % 2], SIGMAS[(a + b) % 3])
       for a, K in enumerate(KS) for b, m in enumerate((K + 1, 2 * K + 5, 1000))]
# every other J and m_new, over K on both sides of the tiles and the row-block switches
SMALL = [(K, m, mnew, J, ("range", "perm")[a % 2], SIGMAS[a % 3])
         for a, (K, m, mnew, J) in enumerate([(16, 37, 1, 1), (17, 18, 15, 2), (64, 1000, 16, 3), (65, 135, 17, 1),
                                              (120, 245, 63, 2), (121, 122, 64, 3), (200, 1000, 65, 2), (129, 263, 1, 3),
                                              (200, 405, 17, 1), (63, 64, 64, 10)])]


@pytest.mark.parametrize("K,m,kind,sig", BIG)
def test_columns_are_the_binary_entry(pair, K, m, kind, sig):
    compare(pair[2], K, m, 300, 10, kind, sig, seed=31 * K + m)


@pytest.mark.parametrize("K,m,mnew,J,kind,sig", SMALL)
def test_columns_are_the_binary_entry_small(pair, K, m, mnew, J, kind, sig):
    compare(pair[2], K, m, mnew, J, kind, sig, seed=37 * K + m + mnew)


def test_a_class_without_a_member(pair):
    idx0, _, Y = problem(500, 300, 10, "perm", 5, empty=4)
    assert not (Y == 4).any() and (Y == 5).any()
    compare(pair[2], 64, 500, 300, 10, "perm", SIGMAS[0], seed=5, empty=4)


def test_sixteen_row_block():
    """K = 205: the fused kernel stages 16 rows per workgroup."""
    _, _, rp = resident(N, 210, 109)
    try:
        compare(rp, 205, 1000, 300, 10, "perm", SIGMAS[0], seed=205)
        compare(rp, 205, 206, 65, 3, "range", SIGMAS[1], seed=206)
    finally:
        rp.free()


# ---- 2. m <= K: the dense route per class --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["range", "perm"])
@pytest.mark.parametrize("K,m", [(50, 40), (200, 200), (65, 1)])
def test_dense_route(pair, K, m, kind):
    for a, mnew in enumerate((300, 17)):
        compare(pair[2], K, m, mnew, 3, kind, SIGMAS[a], seed=K + m)


# ---- 3. the worker count does not show -----------------------------------------------------------------------------------
def test_worker_count_does_not_show(pair):
    _, _, rp = pair
    idx0, idx1, Y = problem(1000, 300, 10, "perm", 3)
    ts = ts_of(10)
    runs = [rp.logit_posterior_multiclass(idx0, idx1, 64, ts, Y, 1e-3, max_parallel=w, return_iters=True) for w in (1, 3, 16, 16, 0)]
    first, its0 = runs[0]
    mean, cov, its_ref = binary_columns(rp, idx0, idx1, 64, ts, Y, 0.0, 1e-3)
    assert_same_bytes(first, its0, mean, cov, its_ref, "max_parallel=1")
    for got, its in runs[1:]:
        assert got["mean"].tobytes() == first["mean"].tobytes() and got["cov"].tobytes() == first["cov"].tobytes()
        assert np.array_equal(its, its0)


# ---- 4. the wide route ---------------------------------------------------------------------------------------------------
def test_wide_route():
    _, _, rp = resident(N, 1025, 111)
    try:
        for w in (1, 2):
            compare(rp, 1025, 1100, 65, 2, "perm", SIGMAS[1], seed=1025, max_parallel=w)
    finally:
        rp.free()


# ---- 5. the convergence protocol per class -------------------------------------------------------------------------------
@pytest.mark.parametrize("K,m", [(64, 1000), (200, 405), (50, 40)])
def test_max_iter_stops_some_classes_and_not_others(pair, K, m):
    _, _, rp = pair
    J, (s11, s22) = 10, SIGMAS[1]
    idx0, idx1, Y = problem(m, 65, J, "perm", 7 * K)
    ts = ts_of(J)
    full = compare(rp, K, m, 65, J, "perm", SIGMAS[1], seed=7 * K)
    assert len(set(full.tolist())) > 1, f"the classes' iteration counts are all {full[0]}: the case says nothing"
    cap = int(full.min())
    mean, cov, its_ref = binary_columns(rp, idx0, idx1, K, ts, Y, s11, s22, max_iter=cap)
    got, its = rp.logit_posterior_multiclass(idx0, idx1, K, ts, Y, s22, sigma11=s11, max_iter=cap, return_iters=True)
    assert_same_bytes(got, its, mean, cov, its_ref, f"max_iter={cap}")
    assert (its == cap).all() and (full > cap).any()


# ---- 6. independent anchor -----------------------------------------------------------------------------------------------
def test_against_the_dense_restatement(pair):
    values, V, rp = pair
    K, m, J, (s11, s22) = 64, 1000, 3, SIGMAS[1]
    idx0, idx1, Y = problem(m, 300, J, "perm", 11)
    ts = ts_of(J)
    got = rp.logit_posterior_multiclass(idx0, idx1, K, ts, Y, s22, sigma11=s11)
    assert (got["cov"] >= s22).all()
    for j in range(J):
        mean, cov, C22, _, _ = ref.dense_posterior(values, V, K, ts[j], idx0, idx1, (Y == j).astype(np.float64), s11, s22, 1e-5)
        atol_mean, atol_cov = ref.tolerances(mean, cov, C22, m)
        dm = np.abs(got["mean"][:, j] - mean).max(); dc = np.abs(got["cov"][:, j] - cov).max()
        print(f"class {j}: |dmean| {dm:.3e} (atol {atol_mean:.3e})  |dcov| {dc:.3e} (atol {atol_cov:.3e})")
        assert dm <= atol_mean and dc <= atol_cov, j


# ---- 7. the score on the resident result ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mnew,J,n_samples", [(1, 2, 1), (300, 10, 100), (4097, 2, 100), (4097, 10, 1), (300, 2, 1), (1, 10, 100)])
def test_nll_is_the_host_entry_on_the_returned_arrays(pair, mnew, J, n_samples):
    _, _, rp = pair
    rng = np.random.default_rng(mnew + J)
    idx0 = rng.permutation(N)[:300]
    idx1 = rng.integers(0, N, mnew)                       # 4097 rows of a 3000-row pair: an index set with repeats
    Y = rng.integers(0, J, 300).astype(np.float64)
    target = rng.integers(0, J, mnew).astype(np.float64); target[0] = J - 1
    ts, seed = ts_of(J), 12345 + mnew
    got = rp.logit_posterior_multiclass(idx0, idx1, 64, ts, Y, 1e-3, target=target, n_samples=n_samples, seed=seed)
    plain = rp.logit_posterior_multiclass(idx0, idx1, 64, ts, Y, 1e-3)
    assert got["mean"].tobytes() == plain["mean"].tobytes() and got["cov"].tobytes() == plain["cov"].tobytes()
    want = api.negative_log_likelihood(got["mean"], got["cov"], target, "multinomial", n_samples, seed)
    assert np.isfinite(want)
    assert np.float64(got["nll"]).tobytes() == np.float64(want).tobytes(), (got["nll"], want)
    only = rp.logit_posterior_multiclass(idx0, idx1, 64, ts, Y, 1e-3, target=target, n_samples=n_samples, seed=seed,
                                         return_posterior=False)
    assert set(only) == {"nll"} and np.float64(only["nll"]).tobytes() == np.float64(want).tobytes()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------
def _raw(rp, nll=False, K=20, J=3, ts=None, m=30, Y=None, mnew=5, s11=0.0, s22=1e-3, max_parallel=4, mean=True, cov=True,
         target=None, n_samples=10, null=()):
    i0 = np.arange(m, dtype=np.int32); i1 = np.arange(100, 100 + max(mnew, 1), dtype=np.int32)
    ts = np.ascontiguousarray(ts_of(max(J, 1)) if ts is None else ts, dtype=np.float64)
    Y = np.ascontiguousarray((np.arange(m) % max(J, 1)) if Y is None else Y, dtype=np.float64)
    mu = np.zeros((max(mnew, 1), max(J, 1)), order="F"); cv = np.zeros((max(mnew, 1), max(J, 1)), order="F")
    p = dict(ts=ts.ctypes.data, idx0=i0.ctypes.data, Y=Y.ctypes.data, idx1=i1.ctypes.data)
    for name in null:
        p[name] = None
    head = (rp._h if rp is not None else None, K, p["ts"], J, s11, s22, p["idx0"], m, p["Y"], p["idx1"], mnew, 1e-5, 100,
            max_parallel, mu.ctypes.data if mean else None, cv.ctypes.data if cov else None, None)
    L = _lib.lib()
    if not nll:
        return L.flgp_eigenpair_logit_posterior_multiclass(*head)
    tg = np.ascontiguousarray((np.arange(max(mnew, 1)) % max(J, 1))[::-1] if target is None else target, dtype=np.float64)
    out = ctypes.c_double()
    return L.flgp_eigenpair_logit_posterior_multiclass_nll(*head, None if "target" in null else tg.ctypes.data, n_samples, 1,
                                                           None if "nll" in null else ctypes.byref(out))


def test_refusals():
    _, _, rp = resident(500, 20, 107)
    L = _lib.lib()
    nan_ts = ts_of(3); nan_ts[1] = np.nan
    inf_ts = ts_of(3); inf_ts[2] = np.inf
    base_Y = (np.arange(30) % 3).astype(np.float64)
    bad = {
        "J = 0": (dict(J=0), "J=0 must be at least 1"),
        "ts nan": (dict(ts=nan_ts), "ts[1]=nan must be finite"),
        "ts inf": (dict(ts=inf_ts), "ts[2]=inf must be finite"),
        "label 1.5": (dict(Y=np.r_[base_Y[:29], 1.5]), "Y[29]=1.5 is not a class label in 0 .. 2"),
        "label -1": (dict(Y=np.r_[-1.0, base_Y[1:]]), "Y[0]=-1 is not a class label in 0 .. 2"),
        "label J": (dict(Y=np.r_[base_Y[:29], 3.0]), "Y[29]=3 is not a class label in 0 .. 2"),
        "sigma11 < 0": (dict(s11=-1e-3), "sigma11=-0.001 must be finite and >= 0"),
        "sigma22 < 0": (dict(s22=-1e-3), "sigma22=-0.001 must be finite and >= 0"),
        "null pair": (dict(rp=None), "null pointer"),
        "null ts": (dict(null=("ts",)), "null pointer"),
        "null idx0": (dict(null=("idx0",)), "null pointer"),
        "null Y": (dict(null=("Y",)), "null pointer"),
        "null idx1": (dict(null=("idx1",)), "null pointer"),
        "K > ep.K": (dict(K=21), "bad shape"),
        "m_new = 0": (dict(mnew=0), "bad shape"),
    }
    for nll in (False, True):
        for m in (30, 10):                       # both routes refuse before any device work
            for name, (kw, text) in bad.items():
                kw = dict(kw)
                r = kw.pop("rp", rp)
                if "Y" in kw and m != 30:
                    continue
                assert _raw(r, nll=nll, m=m, **kw) == -1, name
                msg = L.flgp_last_error().decode()
                assert msg.startswith("logit_posterior_multiclass: ") and text in msg, (name, msg)
            assert _raw(rp, nll=nll, m=m) == 0, L.flgp_last_error().decode()          # a valid call after the refusals
    # the first entry needs both arrays; the score-only entry takes both or neither
    for kw in (dict(mean=False), dict(cov=False), dict(mean=False, cov=False)):
        assert _raw(rp, **kw) == -1 and L.flgp_last_error().decode() == "logit_posterior_multiclass: null pointer"
    for kw in (dict(mean=False), dict(cov=False), dict(null=("target",)), dict(null=("nll",))):
        assert _raw(rp, nll=True, **kw) == -1 and L.flgp_last_error().decode() == "logit_posterior_multiclass: null pointer"
    assert _raw(rp, nll=True, mean=False, cov=False) == 0
    # the target's checks are negative_log_likelihood's, with its texts
    assert _raw(rp, nll=True, target=[0, 1, 1, 0, 1]) == -1
    assert L.flgp_last_error().decode() == "logit_posterior_multiclass: the labels name 2 classes, mean and cov have J=3 columns"
    assert _raw(rp, nll=True, target=[0, 1, 2.5, 0, 1]) == -1
    assert L.flgp_last_error().decode() == "logit_posterior_multiclass: target[2]=2.5 is not a class label in 0 .. 2"
    assert _raw(rp, nll=True, n_samples=0) == -1
    assert L.flgp_last_error().decode() == "logit_posterior_multiclass: n_samples=0 must be at least 1"
    # max_parallel below 1 is clipped, not refused
    assert _raw(rp, max_parallel=0) == 0 and _raw(rp, max_parallel=-3) == 0
    with pytest.raises(api.FlgpError) as e:
        rp.logit_posterior_multiclass(np.arange(30), np.array([0, 500]), 20, ts_of(3), base_Y, 1e-3)
    assert e.value.code == -1 and "idx1[1]=500 out of range" in e.value.message
    post = rp.logit_posterior_multiclass(np.arange(30), np.arange(100, 105), 20, ts_of(3), base_Y, 1e-3)
    assert np.isfinite(post["mean"]).all() and (post["cov"] >= 1e-3).all()
    rp.free()
