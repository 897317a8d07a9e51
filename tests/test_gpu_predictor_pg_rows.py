"""GPU (-m gpu): flgp_dev_predictor_pg_rows and flgp_dev_pg_link (csrc/predictor.hip) alone, on random ELL rows
and a random P in padded, canaried buffers; the padding columns of P are NaN.  Shapes: tests/predictor_pg_cases.py (what they
reach: tests/test_predictor_pg_case_table.py).  Per (r, s, B) the restatement is computed once, on the 257 rows; a call on n
rows must give its first n.

* f is bit for bit the restatement's (tests/np_predictor_pg.py: one chain over a ascending, multiply then add);
* y and label are exactly (pi_dev > 0.5) and the first arg-max of pi_dev;
* |pi_dev - 1 / (1 + exp(-f_dev))| (numpy) <= 8 * 2^-53.  With u = 2^-53 and both exp within 1 ulp (each library's
  documented bound, not measured here) the two values of e = exp(-f) differ by at most 2u e; the denominator 1 + e then by
  2u e / (1 + e) + 2u relative, the two divisions add 2u: <= 6u relative, pi <= 1, 8u leaves a margin.  The largest
  observed ratio to the bound is printed (recorded in DESIGN f-22);
* every subset of the outputs is asked for: the bits of one output do not depend on which others were requested, and what
  was not requested stays untouched;
* flgp_dev_pg_link on f_dev gives the fused outputs bit for bit;
* ties go to the lowest chain (columns 3 and 5 equal; columns 0 and 64 equal; several pi exactly 1.0); f = -800 gives
  pi = 0 without a NaN."""
import functools

import numpy as np
import pytest
import torch

import np_predictor_pg as npg
import predictor_pg_cases as pc
from flgp_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NMAX = max(pc.NS)
U8 = 8.0 * 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _inputs(r, s, B):
    rng = np.random.default_rng([r, s, B])
    if r <= s:
        idx = np.sort(np.stack([rng.permutation(s)[:r] for _ in range(NMAX)]), axis=1).astype(np.int32)
    else:
        idx = np.sort(rng.integers(0, s, size=(NMAX, r)), axis=1).astype(np.int32)                # indices repeat
    val = rng.normal(size=(NMAX, r)) * 10.0 ** rng.uniform(-1.0, 1.0, size=(NMAX, r)) / r        # mixed signs and magnitudes
    ldp = (B + 15) // 16 * 16 + 3
    P = np.full((s, ldp), np.nan)
    P[:, :B] = rng.normal(size=(s, B))
    f = npg.latent(idx, val, P, B)
    for a in (idx, val, P, f):
        a.setflags(write=False)
    return idx, val, P, ldp, f


def _run(idx, val, P, ldp, n, B, want=pc.OUTPUTS):
    """one call on the first n rows; every output sits in NaN with a leading dimension of its own and a spare column.
    Returns {name: n x B (label: n)} of what was asked for"""
    L = _lib.lib()
    r, s = idx.shape[1], P.shape[0]
    d_idx = torch.from_numpy(idx[:n].copy()).to(DEV); d_val = torch.from_numpy(val[:n].copy()).to(DEV)
    d_P = torch.from_numpy(np.array(P)).to(DEV)
    ld = {"f": n + 3, "pi": n + 2, "y": n + 1}
    buf = {k: torch.full((B + 1, ld[k]), float("nan"), dtype=torch.float64, device=DEV) for k in ld}
    lab = torch.full((n + 2,), float("nan"), dtype=torch.float64, device=DEV)
    ptr = {k: (buf[k].data_ptr() if k in want else None) for k in ld}
    rc = L.flgp_dev_predictor_pg_rows(None, d_idx.data_ptr(), d_val.data_ptr(), n, r, d_P.data_ptr(), ldp, s, B, ptr["f"], ld["f"],
                                      ptr["pi"], ld["pi"], ptr["y"], ld["y"], lab.data_ptr() if "label" in want else None)
    assert rc == 0, L.flgp_last_error().decode()
    torch.cuda.synchronize()
    out = {}
    for k in ld:
        a = buf[k].cpu().numpy()
        assert np.isnan(a[:, n:]).all() and np.isnan(a[B:]).all(), k                              # canaries
        if k in want:
            out[k] = a[:B, :n].T
            assert not np.isnan(out[k]).any(), k
        else:
            assert np.isnan(a).all(), k
    a = lab.cpu().numpy()
    assert np.isnan(a[n:]).all()
    if "label" in want:
        out["label"] = a[:n]
    else:
        assert np.isnan(a).all()
    np.testing.assert_array_equal(d_P.cpu().numpy(), P)
    np.testing.assert_array_equal(d_idx.cpu().numpy(), idx[:n]); np.testing.assert_array_equal(d_val.cpu().numpy(), val[:n])
    return out


def _link(f, want=("pi", "y", "label")):
    """flgp_dev_pg_link on f (n x B) in padded buffers"""
    L = _lib.lib()
    n, B = f.shape
    ldf = n + 5
    d_f = torch.full((B, ldf), float("nan"), dtype=torch.float64, device=DEV)
    d_f[:, :n] = torch.from_numpy(np.ascontiguousarray(f.T)).to(DEV)
    ld = {"pi": n + 2, "y": n + 1}
    buf = {k: torch.full((B + 1, ld[k]), float("nan"), dtype=torch.float64, device=DEV) for k in ld}
    lab = torch.full((n + 2,), float("nan"), dtype=torch.float64, device=DEV)
    rc = L.flgp_dev_pg_link(None, d_f.data_ptr(), ldf, n, B, buf["pi"].data_ptr() if "pi" in want else None, ld["pi"],
                            buf["y"].data_ptr() if "y" in want else None, ld["y"], lab.data_ptr() if "label" in want else None)
    assert rc == 0, L.flgp_last_error().decode()
    torch.cuda.synchronize()
    out = {}
    for k in ld:
        a = buf[k].cpu().numpy()
        assert np.isnan(a[:, n:]).all() and np.isnan(a[B:]).all(), k
        if k in want:
            out[k] = a[:B, :n].T
        else:
            assert np.isnan(a).all(), k
    a = lab.cpu().numpy()
    assert np.isnan(a[n:]).all()
    if "label" in want:
        out["label"] = a[:n]
    return out


def _check_link(got, label=""):
    """y and label exact functions of pi_dev; pi_dev against numpy's on f_dev.  Returns the largest |d| / bound"""
    y, lab = npg.labels_of(got["pi"])
    np.testing.assert_array_equal(got["y"], y, err_msg=label)
    np.testing.assert_array_equal(got["label"], lab, err_msg=label)
    d = np.abs(got["pi"] - npg.logistic(got["f"])).max()
    assert d <= U8, (label, d / U8)
    return d / U8


@pytest.mark.parametrize("B", pc.BS)
def test_rows_match_the_restatement_and_the_link(B):
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    worst = 0.0
    for r, s in pc.shapes(B):
        idx, val, P, ldp, f_ref = _inputs(r, s, B)
        got = {}
        for n in pc.NS:
            got[n] = _run(idx, val, P, ldp, n, B)
            np.testing.assert_array_equal(got[n]["f"], f_ref[:n], err_msg=f"f r={r} s={s} n={n}")
            worst = max(worst, _check_link(got[n], f"r={r} s={s} n={n}"))
        for n in pc.NS[:-1]:                                                      # a row does not depend on n or its position
            for k in pc.OUTPUTS:
                np.testing.assert_array_equal(got[NMAX][k][:n], got[n][k], err_msg=f"{k} n={n} against n={NMAX}")
        # the link alone, on the device's f
        for n in (5, NMAX):
            alone = _link(got[n]["f"])
            for k in ("pi", "y", "label"):
                np.testing.assert_array_equal(alone[k], got[n][k], err_msg=f"link {k} r={r} s={s} n={n}")
    print(f"B={B}: largest |pi_dev - numpy| / (8 * 2^-53) = {worst:.3f}")


@pytest.mark.parametrize("B", [2, 65, 130])
def test_every_subset_of_the_outputs(B):
    r, s, n = 5, 7, 5
    idx, val, P, ldp, f_ref = _inputs(r, s, B)
    full = _run(idx, val, P, ldp, n, B)
    for want in pc.SUBSETS:
        got = _run(idx, val, P, ldp, n, B, want)
        assert set(got) == set(want)
        for k in want:
            np.testing.assert_array_equal(got[k], full[k], err_msg=f"{k} of {want}")
    for want in (("pi",), ("y",), ("label",), ("y", "label")):
        got = _link(full["f"], want)
        for k in want:
            np.testing.assert_array_equal(got[k], full[k], err_msg=f"link {k} of {want}")


def _one_hot_rows(P):
    """row i takes row i of P with weight 1: f = P"""
    s = P.shape[0]
    return np.arange(s, dtype=np.int32)[:, None], np.ones((s, 1))


def test_ties_go_to_the_lowest_chain():
    B = 130
    rng = np.random.default_rng(7)
    base = rng.uniform(-2.0, 1.0, size=(6, B))
    P = np.full((6, 144 + 3), np.nan)
    P[:, :B] = base
    P[0, 3] = P[0, 5] = 3.0                                   # columns 3 and 5 equal, one lane each of the same chunk
    P[1, 0] = P[1, 64] = 3.0                                  # columns 0 and 64: the same lane, two chunks
    P[2, 64] = P[2, 65] = P[2, 129] = 3.0                     # a later chunk alone
    P[3, :B] = 40.0 + np.arange(B)                            # pi exactly 1.0 in every chain
    P[4, :B] = -5.0; P[4, 77] = 50.0; P[4, 100] = 60.0        # 1.0 twice
    P[5, :B] = -800.0                                         # pi = 0 everywhere: still the first
    idx, val = _one_hot_rows(P)
    got = _run(idx, val, P, P.shape[1], 6, B)
    np.testing.assert_array_equal(got["f"], P[:, :B])
    np.testing.assert_array_equal(got["label"], [3.0, 0.0, 64.0, 0.0, 77.0, 0.0])
    assert (got["pi"][3] == 1.0).all() and got["pi"][4, 77] == 1.0 and got["pi"][4, 100] == 1.0
    _check_link(got, "ties")
    alone = _link(got["f"])
    for k in ("pi", "y", "label"):
        np.testing.assert_array_equal(alone[k], got[k])


def test_saturation_gives_zero_and_no_nan():
    B = 3
    P = np.full((2, 16), np.nan)
    P[0, :B] = [-800.0, 0.0, 800.0]
    P[1, :B] = [-800.0, -800.0, -745.0]
    idx, val = _one_hot_rows(P)
    got = _run(idx, val, P, 16, 2, B)
    np.testing.assert_array_equal(got["f"], P[:, :B])
    assert got["pi"][0].tolist() == [0.0, 0.5, 1.0] and got["pi"][1, 0] == 0.0 and got["pi"][1, 1] == 0.0
    assert not np.isnan(got["pi"]).any()
    np.testing.assert_array_equal(got["y"], [[0.0, 0.0, 1.0], [0.0, 0.0, 0.0]])
    assert got["label"][0] == 2.0 and got["label"][1] == np.argmax(got["pi"][1])
    _check_link(got, "saturation")
