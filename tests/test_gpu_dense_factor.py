"""GPU: the dense fp64 factorisations under the resident-EigenPair consumers, each on its own stage entry
(include/flgp_hip.h) -- flgp_dev_cholesky (blocked, gpc.hip; one workgroup, gpr.hip), flgp_dev_chol_solve (chol_trsv
modes 1, 2, 3) and flgp_dev_tri_inverse (gpr_grad.hip) -- against numpy / scipy in fp64, at the sizes where the kernels
change behaviour: 64 (panel width of chol_blocked, chol_trsv and tri_inverse), 128 / 256 (workgroup widths) and 1024
(the thread stride of chol_solve_kernel).

Tolerances are first-order error bounds written out per assertion, eps = 2^-52 and gamma(k) = k eps / (1 - k eps)
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.: Thm 8.5 triangular solves, Thm 10.3 and 10.8
Cholesky, sec. 14.2 triangular inverse).  Each is met by any correct fp64 evaluation order and missed by orders of
magnitude by an fp32 path or a dropped block."""
import functools

import numpy as np
import pytest
import scipy.linalg as sl
import torch

from flgp_amd import _lib
from test_gpu_classification import spd, torch_first  # noqa: F401  (torch opens the device first)

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 700, 1023, 1024, 1025, 1100]


def gamma(k):
    return k * EPS / (1.0 - k * EPS)


# ---- test matrices ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def matrix(m, kind):
    """(A, lambda_min, lambda_max): "well" / "ill" = Q diag(d) Q^T with d log-spaced from 1 down to 1e-2 / 1e-8 (Q a
    random orthogonal matrix), "rbf" = the RBF-plus-ridge GP covariance of the classification tests (its spectrum
    computed here)."""
    rng = np.random.default_rng(7919 * m + len(kind))
    if kind == "rbf":
        A, _ = spd(m, rng)
        lam = np.linalg.eigvalsh(A)
        return A, lam[0], lam[-1]
    cond = {"well": 1e2, "ill": 1e8}[kind]
    Q, R = np.linalg.qr(rng.standard_normal((m, m)))
    Q *= np.sign(np.diag(R))
    d = np.logspace(0.0, -np.log10(cond), m) if m > 1 else np.ones(1)
    A = (Q * d) @ Q.T
    return np.asfortranarray(0.5 * (A + A.T)), d.min(), d.max()


def to_dev(a):
    """column-major device copy of a 2-D host array (row-major of a^T)"""
    return torch.tensor(np.ascontiguousarray(a.T), dtype=torch.float64, device="cuda")


def to_host(t):
    return t.cpu().numpy().T.copy()


def flag():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def nan_upper(A):
    """A with its strict upper triangle set to NaN: every entry here reads the lower triangle only"""
    B = np.array(A, dtype=np.float64, order="F")
    B[np.triu_indices(B.shape[0], 1)] = np.nan
    return B


def cholesky(dA, m, single, fl):
    _lib.check(_lib.lib().flgp_dev_cholesky(None, dA.data_ptr(), m, single, fl.data_ptr()))


def chol_solve(dL, m, dB, nrhs, mode, fl):
    _lib.check(_lib.lib().flgp_dev_chol_solve(None, dL.data_ptr(), m, dB.data_ptr(), nrhs, mode, fl.data_ptr()))


def tri_inverse(dL, m, dX, fl):
    L = _lib.lib()
    ws = L.flgp_dev_tri_inverse_workspace(m)
    work = torch.empty(ws // 8, dtype=torch.float64, device="cuda")
    _lib.check(L.flgp_dev_tri_inverse(None, dL.data_ptr(), m, dX.data_ptr(), work.data_ptr(), ws, fl.data_ptr()))
    torch.cuda.synchronize()


# ---- both factorisations ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["well", "rbf"])
@pytest.mark.parametrize("single", [0, 1], ids=["blocked", "one_workgroup"])
@pytest.mark.parametrize("m", SIZES)
def test_cholesky(m, single, kind):
    A, lmin, lmax = matrix(m, kind)
    dA = to_dev(nan_upper(A))
    fl = flag()
    cholesky(dA, m, single, fl)
    torch.cuda.synchronize()
    assert fl.item() == 0
    L = np.tril(to_host(dA))
    assert np.isfinite(L).all()
    # backward error (Thm 10.3): L L^T = A + dA, |dA| <= gamma(m+1) |L||L^T|, and (|L||L^T|)_ij <= sqrt(a_ii a_jj) by
    # Cauchy-Schwarz on rows i, j of L; forming L L^T here adds gamma(m) |L||L^T| more
    s = np.sqrt(np.diag(A))
    res = np.abs(L @ L.T - A) / np.outer(s, s)
    assert res.max() <= gamma(m + 1) + gamma(m), res.max() / (gamma(m + 1) + gamma(m))
    # forward error against LAPACK (Thm 10.8, first order): |dL|_F <= 2^-1/2 kappa(A) |L|_2 |dA|_F / |A|_2 for each
    # factor, |dA|_F <= gamma(m+1) tr(A) from the bound above; the two factors' errors add
    L_ref = np.linalg.cholesky(A)
    bound = np.sqrt(2.0) * (lmax / lmin) * np.sqrt(lmax) * gamma(m + 1) * np.trace(A) / lmax
    err = np.linalg.norm(L - L_ref)
    assert err <= bound, (err, bound)


# ---- chol_trsv, modes 1, 2, 3 separately -----------------------------------------------------------------------------
@pytest.mark.parametrize("nrhs", [0, 1, 3, 65, 300])
@pytest.mark.parametrize("m", SIZES)
def test_chol_solve_modes(m, nrhs):
    A, lmin, _ = matrix(m, "well")
    L = np.linalg.cholesky(A)
    dL = to_dev(nan_upper(L))
    fl = flag()
    rng = np.random.default_rng(m * 1000 + nrhs)
    if nrhs == 0:
        B = rng.standard_normal((m, 2))
        dB = to_dev(B)
        for mode in (1, 2, 3):
            chol_solve(dL, m, dB, 0, mode, fl)
        torch.cuda.synchronize()
        assert np.array_equal(to_host(dB), B)            # bit for bit: nothing ran
        return
    B = rng.standard_normal((m, nrhs))
    nLF, inv_smin = np.linalg.norm(L), 1.0 / np.sqrt(lmin)   # sigma_min(L)^2 = lambda_min(L L^T) = lambda_min(A) to O(eps)
    refs = {1: sl.solve_triangular(L, B, lower=True),
            2: sl.solve_triangular(L, B, lower=True, trans="T"),
            3: sl.cho_solve((L, True), B)}
    # per column (Thm 8.5): (L + dL) x = b with |dL| <= gamma(m) |L|, so |dL|_2 <= gamma(m) |L|_F and
    # |x - x_ref| <= |L^-1|_2 |dL|_2 |x| for each of the two solutions (modes 1, 2); mode 3 runs two such solves,
    # (L L^T + dA) x = b with |dA|_2 <= (2 gamma(m) + gamma(m)^2) |L|_F^2 and |x - x_ref| <= |A^-1|_2 |dA|_2 |x|, twice
    g = gamma(m)
    rel = {1: 2 * g * nLF * inv_smin, 2: 2 * g * nLF * inv_smin, 3: 2 * (2 * g + g * g) * nLF ** 2 * inv_smin ** 2}
    for mode in (1, 2, 3):
        dB = to_dev(B)
        chol_solve(dL, m, dB, nrhs, mode, fl)
        torch.cuda.synchronize()
        X, Xr = to_host(dB), refs[mode]
        err = np.linalg.norm(X - Xr, axis=0) / np.linalg.norm(Xr, axis=0)
        assert err.max() <= rel[mode], (mode, err.max(), rel[mode])
    assert fl.item() == 0


# ---- tri_inverse ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["well", "ill"])
@pytest.mark.parametrize("m", SIZES)
def test_tri_inverse(m, kind):
    A, lmin, lmax = matrix(m, kind)
    dL = to_dev(A)                                          # the factor as flgp_dev_cholesky leaves it (upper: scratch)
    fl = flag()
    cholesky(dL, m, 0, fl)
    dX = torch.full((m, m), 3.0, dtype=torch.float64, device="cuda")
    tri_inverse(dL, m, dX, fl)
    assert fl.item() == 0
    L, X = np.tril(to_host(dL)), to_host(dX)
    assert np.all(X[np.triu_indices(m, 1)] == 0.0)
    nL, nX = np.linalg.norm(L), np.linalg.norm(X)
    # residual (sec. 14.2): |L X - I|_F <= m eps |L|_F |X|_F for the blocked inverse, plus gamma(m) |L|_F |X|_F for
    # forming L X here
    res = np.linalg.norm(L @ X - np.eye(m))
    assert res <= (m * EPS + gamma(m)) * nL * nX, res / (nL * nX)
    # forward error: each of the two inverses is within m eps kappa(L) |X| of L^-1, kappa_2(L) = sqrt(kappa_2(A))
    X_ref = sl.solve_triangular(L, np.eye(m), lower=True)
    err = np.linalg.norm(X - X_ref) / np.linalg.norm(X_ref)
    assert err <= 2 * m * EPS * np.sqrt(lmax / lmin), err


# ---- a refused factorisation: the pivot index, and the solves that must not run ---------------------------------------
@pytest.mark.parametrize("p", [0, 63, 64, 130])
def test_pivot_reporting(p):
    """The leading p x p block of A is the last positive definite one: A[p, p] is set so that the Schur pivot there is
    -1.  The blocked factorisation reports p + 1, the one-workgroup one 1; chol_solve and tri_inverse then run nothing
    (B bit for bit untouched, X = 0)."""
    m = 200
    A, _, _ = matrix(m, "well")
    A = A.copy(order="F")
    A[p, p] = (A[p, :p] @ np.linalg.solve(A[:p, :p], A[:p, p]) if p else 0.0) - 1.0
    if p:
        np.linalg.cholesky(A[:p, :p])                       # still SPD
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(A[:p + 1, :p + 1])
    rng = np.random.default_rng(p)
    B = rng.standard_normal((m, 3))
    for single, want in ((0, p + 1), (1, 1)):
        dA = to_dev(A)
        fl = flag()
        cholesky(dA, m, single, fl)
        torch.cuda.synchronize()
        assert fl.item() == want
        assert np.isfinite(to_host(dA)).all()
        for mode in (1, 2, 3):
            dB = to_dev(B)
            chol_solve(dA, m, dB, 3, mode, fl)
            torch.cuda.synchronize()
            assert np.array_equal(to_host(dB), B), mode
        dX = torch.full((m, m), 3.0, dtype=torch.float64, device="cuda")
        tri_inverse(dA, m, dX, fl)
        assert np.all(to_host(dX) == 0.0)
        assert fl.item() == want


# ---- determinism ------------------------------------------------------------------------------------------------------
def test_determinism():
    m = 1025
    A, _, _ = matrix(m, "rbf")
    B = np.random.default_rng(3).standard_normal((m, 5))
    outs = []
    for _ in range(2):
        fl = flag()
        d0, d1 = to_dev(A), to_dev(A)
        cholesky(d0, m, 0, fl)
        cholesky(d1, m, 1, fl)
        dB = to_dev(B)
        chol_solve(d0, m, dB, 5, 3, fl)
        dX = torch.empty((m, m), dtype=torch.float64, device="cuda")
        tri_inverse(d0, m, dX, fl)
        assert fl.item() == 0
        outs.append([to_host(t) for t in (d0, d1, dB, dX)])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
