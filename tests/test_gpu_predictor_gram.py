"""GPU (-m gpu): flgp_dev_predictor_gram (csrc/predictor_update.hip) alone, on random ELL rows in padded,
canaried buffers: P is NaN outside its K + q columns (ldp = K + q + 5), S sits in NaN with lds = K + q + 3 and a spare column,
the workspace has a NaN tail, Y has ldy = n + 2 with NaN below its rows.  Shapes: tests/predictor_update_cases.py (what they
reach: tests/test_predictor_update_case_table.py).

* Exact on integers: val in {0, 1, 2}, P in [-4, 4], Y in [-8, 8], w in {1, 2, 4}, so |e| <= 264, every term is below 2^19 and a
  sum over n <= 2^14 rows stays below 2^53: the reference is exact in any order and S must equal it bit for bit, on every shape.
* The documented order, on N(0, 1) data of mixed magnitudes: for n <= GC the lower triangle of S is bit for bit flgp_dev_gemm
  without a workspace on A = (w E)^T, B = E, with E from flgp_dev_predictor_cols plus the subtraction and the scaling on the
  host; for n > GC it is 0.0 plus those per-chunk products in ascending order.  Separately, and whatever the order,
  |S - S_ld| <= (n + 4) 2^-53 sum_i |w_i e_ik e_il| against long double: n additions and the product's rounding.
* Repeatability: a second call gives the same bits, S equals its transpose bit for bit, inputs and canaries are untouched; three
  chunks taken as 3, 2 and 1 launches (knob predictor_gram_launch_chunks) give the same bits."""
import functools

import numpy as np
import pytest
import torch

import np_predictor_update as npu
import predictor_update_cases as uc
from flgp_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NMAX = max(uc.NS)
U53 = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _ell(r, s, integers):
    rng = np.random.default_rng([r, s, int(integers)])
    if r <= s:
        idx = np.sort(np.stack([rng.permutation(s)[:r] for _ in range(NMAX)]), axis=1).astype(np.int32)
    else:
        idx = np.sort(rng.integers(0, s, size=(NMAX, r)), axis=1).astype(np.int32)                # indices repeat
    if integers:
        val = rng.integers(0, 3, size=(NMAX, r)).astype(np.float64)
        w = 2.0 ** rng.integers(0, 3, size=NMAX)
    else:
        val = rng.normal(size=(NMAX, r)) * 10.0 ** rng.uniform(-1.0, 1.0, size=(NMAX, r)) / r    # mixed signs and magnitudes
        w = 1.0 / rng.uniform(0.01, 2.0, size=NMAX)
    for a in (idx, val, w):
        a.setflags(write=False)
    return idx, val, w


@functools.lru_cache(maxsize=None)
def _operand(s, K, q, integers):
    rng = np.random.default_rng([s, K, q, int(integers)])
    W = K + q
    P = np.full((s, W + uc.LDP_PAD), np.nan)
    Y = np.full((q, NMAX + 2), np.nan)                                                           # column-major n x q at ldy = NMAX + 2
    if integers:
        P[:, :W] = rng.integers(-4, 5, size=(s, W)); Y[:, :NMAX] = rng.integers(-8, 9, size=(q, NMAX))
    else:
        P[:, :W] = rng.normal(size=(s, W)) * 10.0 ** rng.uniform(-1.0, 1.0, size=(1, W)); Y[:, :NMAX] = rng.normal(size=(q, NMAX))
    P.setflags(write=False); Y.setflags(write=False)
    return P, Y


class _Dev:
    def __init__(self, idx, val, w, P, Y):
        up = lambda a: torch.from_numpy(np.array(a)).to(DEV)
        self.idx, self.val, self.w, self.P, self.Y = up(idx), up(val), up(w), up(P), up(Y)
        self.host = (idx, val, w, P, Y)

    def untouched(self):
        for d, h in zip((self.idx, self.val, self.w, self.P, self.Y), self.host):
            np.testing.assert_array_equal(d.cpu().numpy(), h)


def _run(D, n, r, s, K, q, knob=uc.LAUNCH_CHUNKS):
    """one call on rows [0, n); returns S (K + q) x (K + q).  knob: predictor_gram_launch_chunks as it is set"""
    L = _lib.lib()
    W = K + q
    lds = W + uc.LDS_PAD
    need = L.flgp_dev_predictor_gram_workspace(n, K, q)
    assert need == uc.workspace_bytes(n, K, q, knob)
    S = torch.full((W + 1, lds), float("nan"), dtype=torch.float64, device=DEV)
    work = torch.full((need // 8 + 64,), float("nan"), dtype=torch.float64, device=DEV)
    rc = L.flgp_dev_predictor_gram(None, D.idx.data_ptr(), D.val.data_ptr(), n, r, D.P.data_ptr(), W + uc.LDP_PAD, s, K, q, D.w.data_ptr(),
                                   D.Y.data_ptr(), NMAX + 2, S.data_ptr(), lds, work.data_ptr(), need)
    assert rc == 0, L.flgp_last_error().decode()
    torch.cuda.synchronize()
    a = S.cpu().numpy()
    assert np.isnan(a[:, W:]).all() and np.isnan(a[W:]).all()                                     # canaries of S
    assert torch.isnan(work[need // 8:]).all().item()                                             # and of the workspace
    return a[:W, :W].T                                                                            # column-major


@pytest.mark.parametrize("K,q", uc.KQS)
def test_exact_on_integers(K, q):
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    for r in uc.RS:
        for s in uc.SS:
            idx, val, w = _ell(r, s, True)
            P, Y = _operand(s, K, q, True)
            D = _Dev(idx, val, w, P, Y)
            E = npu.rows_e(idx, val, P, K, q, Y[:, :NMAX].T)
            assert np.abs(E).max() <= 264
            for n in uc.NS:
                got = _run(D, n, r, s, K, q)
                np.testing.assert_array_equal(got, npu.gram_int(E[:n], w[:n]), err_msg=f"r={r} s={s} K={K} q={q} n={n}")
            D.untouched()


def _gemm_chunk(Ew, E):
    """flgp_dev_gemm without a workspace: C = Ew^T E, (K + q) x (K + q), for the rows of one chunk (C-ordered n x W operands)"""
    L = _lib.lib()
    n, W = E.shape
    dA, dB = torch.from_numpy(np.ascontiguousarray(Ew)).to(DEV), torch.from_numpy(np.ascontiguousarray(E)).to(DEV)
    C = torch.zeros((W, W), dtype=torch.float64, device=DEV)
    rc = L.flgp_dev_gemm(None, W, W, n, 1.0, dA.data_ptr(), 1, W, dB.data_ptr(), W, 1, 0.0, None, 0, 0, C.data_ptr(), W, 1, None, 0)
    assert rc == 0, L.flgp_last_error().decode()
    torch.cuda.synchronize()
    return C.cpu().numpy()                                                                        # C[k, l]


def _device_e(D, n, r, s, K, q, Y):
    L = _lib.lib()
    W = K + q
    out = torch.zeros((W, n), dtype=torch.float64, device=DEV)
    rc = L.flgp_dev_predictor_cols(None, D.idx.data_ptr(), D.val.data_ptr(), n, r, D.P.data_ptr(), W + uc.LDP_PAD, s, 0, W, out.data_ptr(), n)
    assert rc == 0, L.flgp_last_error().decode()
    torch.cuda.synchronize()
    E = out.cpu().numpy().T.copy()
    E[:, K:] = Y[:, :n].T - E[:, K:]
    return E


@pytest.mark.parametrize("r,s,K,q,n", uc.ORDER_CASES)
def test_the_documented_order_and_the_bound(r, s, K, q, n):
    idx, val, w = _ell(r, s, False)
    P, Y = _operand(s, K, q, False)
    D = _Dev(idx, val, w, P, Y)
    got = _run(D, n, r, s, K, q)
    E = _device_e(D, n, r, s, K, q, Y)
    np.testing.assert_array_equal(E, npu.rows_e(idx[:n], val[:n], P, K, q, Y[:, :n].T))           # the chain of the row kernels
    Ew = w[:n, None] * E
    ref = np.zeros((K + q, K + q))
    for i0, i1 in npu.chunks(n):
        ref = ref + _gemm_chunk(Ew[i0:i1], E[i0:i1])
    low = np.tril_indices(K + q)
    np.testing.assert_array_equal(got[low], ref[low], err_msg="the lower triangle is the chain of flgp_dev_gemm per chunk, chunks ascending")
    np.testing.assert_array_equal(got, got.T)
    S_ld, A_ld = npu.gram_ld(E, w[:n])
    ratio = float((np.abs(got.astype(npu.LD) - S_ld)[low] / ((n + 4) * npu.LD(U53) * A_ld[low])).max())
    print(f"r={r} s={s} K={K} q={q} n={n}: |S - S_ld| / ((n + 4) u sum |terms|) = {ratio:.3e}")
    assert ratio <= 1.0
    np.testing.assert_array_equal(_run(D, n, r, s, K, q), got)                                     # a second call: the same bits
    D.untouched()


@pytest.mark.parametrize("K,q", [(14, 3), (127, 3)])
def test_the_launches_continue_one_chain(K, q):
    """three chunks as 3, 2 and 1 launches: the same bits, from a workspace of 1, 2 and 3 chunks"""
    r, s, n = 5, 300, max(uc.NS)
    idx, val, w = _ell(r, s, False)
    P, Y = _operand(s, K, q, False)
    D = _Dev(idx, val, w, P, Y)
    L = _lib.lib()
    want = _run(D, n, r, s, K, q)
    try:
        for knob in (1, 2):
            assert uc.launches(n, K, q, knob) == 4 - knob
            L.flgp_set_tuning(b"predictor_gram_launch_chunks", knob)
            np.testing.assert_array_equal(_run(D, n, r, s, K, q, knob), want)
    finally:
        L.flgp_set_tuning(b"predictor_gram_launch_chunks", uc.LAUNCH_CHUNKS)
    D.untouched()


@pytest.mark.parametrize("K,q", [(14, 3), (127, 3)])
def test_repeatable_and_symmetric_at_every_n(K, q):
    r, s = 5, 300
    idx, val, w = _ell(r, s, False)
    P, Y = _operand(s, K, q, False)
    D = _Dev(idx, val, w, P, Y)
    for n in uc.NS:
        a, b = _run(D, n, r, s, K, q), _run(D, n, r, s, K, q)
        np.testing.assert_array_equal(a, b); np.testing.assert_array_equal(a, a.T)
        assert np.isfinite(a).all()
    D.untouched()
