"""GPU: B Polya-Gamma chains in one call (flgp_eigenpair_pg_predict_batch).  The contract is bits: column b
of every output equals what the single entry returns for chain b's (column, t, seed), whatever B, the order, the chunk size
or the other chains are -- every comparison with the single entry is np.array_equal.  The single and the one-vs-rest entry
are the batch of one and of J, so these comparisons show that a chain's bits do not depend on its company; what the two
returned while they ran a sweep of their own is pinned in tests/golden/pg_predict_bits.npz (test_gpu_pg_bits.py).  One test
holds the batch to the numpy restatement (tests/np_pg.py) instead, at the bound the single entry is held to, so that the
suite does not rest on one implementation alone."""
import os
import re
import sys

import numpy as np
import pytest

from flgp_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_pg  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the panel width of chol_blocked / lrb_chol (flgp_amd/csrc/gpc.hip): a K one past it takes a second panel, a column block
# and a trailing product in every slot's factorisation
CNB = int(re.search(r"constexpr int CNB = (\d+);", open(os.path.join(ROOT, "flgp_amd", "csrc", "gpc.hip")).read()).group(1))
KEYS = ("pi_pred", "Y_pred", "omega", "f")


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its own HIP runtime: it has to open the device before libflgp_hip.so does."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    torch.cuda.init()


def synthetic_pair(n, K, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
    V = np.asfortranarray(scale * rng.standard_normal((n, K)))
    return api.EigenPair(values, V), api.ResidentEigenPair.from_host(api.EigenPair(values, V))


_pairs = {}


def pair(cols=40):
    """One resident pair of 500 rows per width for the whole module (never written to)."""
    if cols not in _pairs:
        _pairs[cols] = synthetic_pair(500, cols, seed=1600 + cols, scale=0.5)
    return _pairs[cols]


def problem(m, ncol, seed, overlap=True):
    """Training rows, new rows that overlap them (so that sigma_nv's match term has entries) and ncol label columns."""
    rng = np.random.default_rng(seed)
    idx0 = rng.choice(500, m, replace=False).astype(np.int32)
    idx1 = np.arange(0, 500, 3, dtype=np.int32) if overlap else np.setdiff1d(np.arange(500, dtype=np.int32), idx0)[::3]
    Y = np.asfortranarray((rng.uniform(size=(m, ncol)) < 0.45).astype(float))
    return idx0, idx1, Y


def single(rp, idx0, idx1, K, t, y, sigma, sigma_nv, ns, seed):
    return rp.test_pgbinary(idx0, idx1, K, t, y, sigma, sigma_nv, N_sample=ns, output_pi=True, seed=seed, return_state=True)


def batch(rp, idx0, idx1, K, ts, Y, sigma, sigma_nv, ns, col, seeds, max_parallel=0):
    return rp.test_pgbinary_batch(idx0, idx1, K, ts, Y, sigma, sigma_nv, col=col, seeds=seeds, N_sample=ns,
                                  max_parallel=max_parallel, output_pi=True, return_state=True)


def assert_chains_are_single(rp, idx0, idx1, K, ts, Y, sigma, sigma_nv, ns, col, seeds, out):
    for b in range(len(ts)):
        ref = single(rp, idx0, idx1, K, ts[b], Y[:, col[b]], sigma, sigma_nv, ns, seeds[b])
        for k in KEYS:
            assert np.array_equal(out[k][:, b], ref[k]), (b, k)


# ---- 1. each chain is the single entry ----------------------------------------------------------------------------------
SHAPES = [(40, 24),            # the m x m route
          (40, 40),            # m = K: still m x m
          (40, 41),            # the first Woodbury shape
          (16, 48), (8, 64),   # the Woodbury shapes of tests/test_gpu_pg.py
          (12, 257),           # crosses the 256-thread block; m is no multiple of 32, so the slot strides are padded
          (33, 300),           # K is no multiple of 32
          (CNB + 1, CNB + 2)]  # one column past lrb_chol's panel


@pytest.mark.parametrize("K,m", SHAPES)
def test_each_chain_is_the_single_entry(K, m):
    _, rp = pair(40 if K <= 40 else K)
    idx0, idx1, Y = problem(m, 3, seed=K * 1000 + m)
    ts = [1.5, 4.0, 2.25, 3.0, 2.25]; col = [2, 0, 1, 0, 2]; seeds = [11, 2 ** 63 + 5, 77, 12, 2 ** 64 - 1]
    sigma, sigma_nv = 2e-2, 1e-2
    assert np.intersect1d(idx0, idx1).size > 0
    out = batch(rp, idx0, idx1, K, ts, Y, sigma, sigma_nv, 6, col, seeds)
    assert_chains_are_single(rp, idx0, idx1, K, ts, Y, sigma, sigma_nv, 6, col, seeds, out)


# ---- 2. any B ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 7, 33])
def test_any_number_of_chains(B):
    _, rp = pair()
    K, m = 16, 48
    idx0, idx1, Y = problem(m, 4, seed=B)
    rng = np.random.default_rng(100 + B)
    ts = rng.uniform(1.5, 4.0, B); col = rng.integers(0, 4, B); seeds = [int(s) for s in rng.integers(0, 2 ** 62, B)]
    out = batch(rp, idx0, idx1, K, ts, Y, 1e-2, 5e-3, 3, col, seeds)
    assert out["pi_pred"].shape == (idx1.size, B) and out["omega"].shape == (m, B)
    assert_chains_are_single(rp, idx0, idx1, K, ts, Y, 1e-2, 5e-3, 3, col, seeds, out)


# ---- 3. company, order, chunks ------------------------------------------------------------------------------------------
def seven(K, m):
    idx0, idx1, Y = problem(m, 3, seed=K + m)
    ts = np.array([1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 1.75]); col = np.array([0, 1, 2, 0, 1, 2, 1])
    seeds = [901, 902, 903, 904, 905, 906, 907]
    return idx0, idx1, Y, ts, col, seeds


def test_a_permutation_of_the_chains_permutes_the_columns():
    _, rp = pair()
    K, m = 12, 60
    idx0, idx1, Y, ts, col, seeds = seven(K, m)
    base = batch(rp, idx0, idx1, K, ts, Y, 1e-2, 5e-3, 4, col, seeds)
    p = np.array([4, 0, 6, 2, 5, 1, 3])
    perm = batch(rp, idx0, idx1, K, ts[p], Y, 1e-2, 5e-3, 4, col[p], [seeds[i] for i in p])
    for k in KEYS:
        assert np.array_equal(perm[k], base[k][:, p]), k


@pytest.mark.parametrize("K,m", [(12, 60), (24, 20)])          # Woodbury chunks; the m x m route's workers
def test_the_chunk_size_does_not_change_a_bit(K, m):
    _, rp = pair()
    idx0, idx1, Y, ts, col, seeds = seven(K, m)
    base = batch(rp, idx0, idx1, K, ts, Y, 1e-2, 5e-3, 4, col, seeds, max_parallel=0)
    for mp in (1, 2, 3):                                        # 7 chains: the last chunk is ragged
        out = batch(rp, idx0, idx1, K, ts, Y, 1e-2, 5e-3, 4, col, seeds, max_parallel=mp)
        for k in KEYS:
            assert np.array_equal(out[k], base[k]), (mp, k)
    assert_chains_are_single(rp, idx0, idx1, K, ts[:2], Y, 1e-2, 5e-3, 4, col[:2], seeds[:2],
                             {k: base[k][:, :2] for k in KEYS})


def test_duplicates_repeats_and_seeds():
    _, rp = pair()
    K, m = 12, 60
    idx0, idx1, Y, ts, col, seeds = seven(K, m)
    ts = ts.copy(); col = col.copy()
    ts[5], col[5], seeds[5] = ts[1], col[1], seeds[1]           # chain 5 is chain 1 again
    a = batch(rp, idx0, idx1, K, ts, Y, 1e-2, 5e-3, 4, col, seeds)
    for k in KEYS:
        assert np.array_equal(a[k][:, 5], a[k][:, 1]), k
    b = batch(rp, idx0, idx1, K, ts, Y, 1e-2, 5e-3, 4, col, seeds)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    other = list(seeds); other[3] += 1000
    c = batch(rp, idx0, idx1, K, ts, Y, 1e-2, 5e-3, 4, col, other)
    assert not np.array_equal(c["omega"][:, 3], a["omega"][:, 3])
    for k in KEYS:                                              # and only that chain moved
        assert np.array_equal(np.delete(c[k], 3, axis=1), np.delete(a[k], 3, axis=1)), k


# ---- 4. N_sample edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [1, 20])
def test_n_sample_edges(ns):
    _, rp = pair()
    K, m = 16, 48
    idx0, idx1, Y = problem(m, 3, seed=ns)
    ts = [1.5, 2.5, 4.0]; col = [0, 1, 2]; seeds = [5, 6, 7]
    out = batch(rp, idx0, idx1, K, ts, Y, 1e-2, 1e-2, ns, col, seeds)
    assert_chains_are_single(rp, idx0, idx1, K, ts, Y, 1e-2, 1e-2, ns, col, seeds, out)


# ---- 5. independent of the single entry ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K,m", [(16, 48), (40, 24)])
def test_batch_reproduces_numpy(K, m):
    """omega, f and pi against the numpy restatement fed with the same random numbers, at rtol = atol = 1e-9: the bound
    tests/test_gpu_pg.py::test_resident_chain_reproduces_numpy holds the single entry to."""
    ep, rp = pair()
    idx0, idx1, Y = problem(m, 3, seed=K * 7 + m)
    ts = [3.0, 1.5, 2.5]; seeds = [1234, 99, 4321]; sigma, ns = 1e-2, 20
    out = rp.test_pgbinary_batch(idx0, idx1, K, ts, Y, sigma, sigma, seeds=seeds, N_sample=ns, output_pi=True, return_state=True)
    V1 = ep.vectors[idx0, :K]
    for b in range(3):
        l, ls = np_pg.weights(ep.values, K, ts[b])
        omega, f, kappa, C, _ = np_pg.chain(Y[:, b], ns, seeds[b], sigma=sigma, V1=V1, l=l, ls=ls)
        np.testing.assert_allclose(out["omega"][:, b], omega, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(out["f"][:, b], f, rtol=1e-9, atol=1e-9)
        w = np_pg.collapsed_w(omega, kappa, C)
        Cnv = (ep.vectors[idx1, :K] * l) @ V1.T + sigma * (idx1[:, None] == idx0[None, :])
        np.testing.assert_allclose(out["pi_pred"][:, b], np_pg.logistic(Cnv @ w), rtol=1e-9, atol=1e-9)
        assert np.array_equal(out["Y_pred"][:, b], (out["pi_pred"][:, b] > 0.5).astype(float))


# ---- 6. the multiclass wrapper ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,m", [(24, 20), (12, 60)])
def test_multiclass_wrapper_is_the_existing_entry(K, m):
    _, rp = pair()
    idx0, idx1, _ = problem(m, 1, seed=K + 3 * m)
    Y = np.random.default_rng(32 + m).integers(0, 3, m).astype(float)
    sigma, seed = 1e-2, 500
    for ts in (np.array([1.5, 2.5, 4.0]), np.array([1.5, 2.5, 4.0, 3.0])):      # the second: class 3 has no member
        labels, probs = rp.predict_logit_mult_gp_cpp(idx0, idx1, K, ts, Y, sigma, N_sample=15, seed=seed, output_probs=True)
        lb, pb = rp.predict_logit_mult_gp_batch(idx0, idx1, K, ts, Y, sigma, N_sample=15, seed=seed, output_probs=True)
        assert np.array_equal(pb, probs) and np.array_equal(lb, labels)
        assert np.array_equal(lb, np.argmax(pb, axis=1).astype(float))        # numpy's argmax is the first one too
        assert np.array_equal(rp.predict_logit_mult_gp_batch(idx0, idx1, K, ts, Y, sigma, N_sample=15, seed=seed), labels)
    # ties: two chains with the same (column, t, seed) have equal columns, and the first of them is named
    aug = np.asfortranarray(api.multi_train_split(Y))
    out = rp.test_pgbinary_batch(idx0, idx1, K, [2.0, 2.0], aug, sigma, 0.0, col=[1, 1], seeds=[9, 9], N_sample=3,
                                 output_pi=True, return_argmax=True)
    assert np.array_equal(out["argmax"], np.zeros(idx1.size))


# ---- 7. errors that need a pair -----------------------------------------------------------------------------------------
def test_errors_that_need_a_pair():
    _, rp = pair()
    Y = np.array([[0.0, 1.0], [1.0, 0.0], [1.0, 1.0]])
    with pytest.raises(api.FlgpError) as e:
        rp.test_pgbinary_batch([0, 1, 2], [5], 41, [1.0, 2.0], Y, 1e-2, 0.0, seed=1)
    assert e.value.code == -1 and e.value.message == "eigenpair_pg_predict_batch: need 1 <= K <= 40 (K=41)"
    with pytest.raises(api.FlgpError) as e:
        rp.test_pgbinary_batch([0, 1, 500], [5], 10, [1.0, 2.0], Y, 1e-2, 0.0, seed=1)
    assert e.value.code == -1 and e.value.message == "eigenpair_pg_predict_batch: idx0[2]=500 out of range"
    with pytest.raises(api.FlgpError) as e:
        rp.test_pgbinary_batch([0, 1, 2], [5, -1], 10, [1.0, 2.0], Y, 1e-2, 0.0, seed=1)
    assert e.value.code == -1 and e.value.message == "eigenpair_pg_predict_batch: idx1[1]=-1 out of range"
