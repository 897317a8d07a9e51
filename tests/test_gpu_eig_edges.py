"""GPU: flgp_dev_eig_topk at its block-width, Jacobi-plan and stride edges, against LAPACK.

The solver picks its kernels from (s, K) alone.  eig_cases.plan restates those decisions; test_eig_case_table.py (CPU) shows
with it that the tables reach every path, and here flgp_dev_eig_plan -- computed by the functions the solve itself calls -- must
agree with the restatement on every case that runs.

Every case goes through the public entry.  G lies column-major with its leading dimension in a buffer of NaN; the values, the
vectors and the workspace lie in buffers of canaries (eig_cases.Placement), the workspace filled with them too: a slot outside
the K values, outside the K x s block of V or behind flgp_dev_eig_workspace(s, K) bytes must hold its canary bit for bit
afterwards, every slot of the results must be finite.  Each case is solved twice: the solver is deterministic by design, so the
two results are the same bits.

Reference: numpy.linalg.eigh of the same float64 G, once per matrix (eig_cases.problem).  LAPACK reproduces the constructed
spectra to 4e-15 relative at s = 2300, far inside the bars, which are test_gpu_parity.py's own, scaled by lambda_1 where the
matrix is scaled: eigenvalues to 1e-10 relative + 1e-13 lambda_1, V^T V = I to 1e-10, max |G V - V L| < 1e-9 lambda_1, the
invariant subspace within 1e-7 of LAPACK's where the gap below lambda_K exceeds 1e-6 lambda_1.

A truncated solve of the default spectrum must take at least three outer iterations: by EigSolver::iteration a late
Rayleigh-Ritz step then went through jacobi_refine, so the refinement route the plan names did run.

Measured on an MI355X (the whole file: 8 s).  Outer iterations of the truncated default cases, in the table's order: 5, 6, 7, 7,
6, 7, 8, 6, 6, 8, 7, 7, 8, 9; the block-sparse cases and their twin 8 each.  Every
orthonormalisation of those went through Newton-Schulz (info[3] = 1000 x (iterations + 1 or + 2)); only the three truncated
rank-deficient cases used the Jacobi one, once each ((300, 20) then stops after 2 iterations with 11 products).  No case
ended in the fallback, and no seed or spectrum had to be changed (eig_cases.SEEDS is empty).  Filling the workspace with
NaN canaries found one bug: bsg_setup looked at the cluster weights before it looked at "too dense for the CSR", when no
kernel has written them, and refused a dense finite G at s >= 1536 whose workspace happened to hold a NaN there."""
import ctypes
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eig_cases as E  # noqa: E402
from flgp_amd import _lib  # noqa: E402
from flgp_amd.pipeline import HipStages  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EIG_RTOL = 1e-10       # eigenvalues, relative (test_gpu_parity.py)


@pytest.fixture(scope="module")
def stages():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    return HipStages(DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


def device_plan(L, s, K):
    out = (ctypes.c_int * 8)()
    _lib.check(L.flgp_dev_eig_plan(s, K, ctypes.addressof(out)))
    return list(out)


def solve(L, G, K, ldg, ldv, tol=0.0, check=True):
    """one call on fresh buffers: (rc, Placement, info dict)"""
    s = G.shape[0]
    wb = L.flgp_dev_eig_workspace(s, K)
    pl = E.Placement(G, K, ldg, ldv, wb, DEV)
    info = (ctypes.c_int * 4)(-1, -1, -1, -1)
    rc = L.flgp_dev_eig_topk(stream(), pl.G.data_ptr(), ldg, s, K, float(tol), pl.values.data_ptr(), pl.V.data_ptr(), ldv,
                             pl.work.data_ptr(), wb, ctypes.addressof(info))
    if check:
        _lib.check(rc)
    torch.cuda.synchronize()
    return rc, pl, dict(outer_iterations=info[0], g_products=info[1], dense=bool(info[2]), newton_schulz_orths=info[3] // 1000,
                        jacobi_orths=info[3] % 1000)


def accuracy(G, w, Vref, K, lam1, eig, V):
    """the four bars against the reference; returns (messages, figures)"""
    s = G.shape[0]
    bad = []
    verr = np.abs(eig - w[:K]) / (EIG_RTOL * np.abs(w[:K]) + 1e-13 * lam1)
    orth = np.abs(V.T @ V - np.eye(K)).max()
    resid = np.abs(G @ V - V * eig).max() / lam1
    if not verr.max() <= 1.0:
        bad.append(f"eigenvalues: {verr.max():.3g} of the bar at position {int(verr.argmax())}")
    if not orth <= 1e-10:
        bad.append(f"V^T V - I: {orth:.3g}")
    if not resid < 1e-9:
        bad.append(f"max |G V - V L| / lambda_1: {resid:.3g}")
    sub = None
    if K < s and w[K - 1] - w[K] > 1e-6 * lam1:
        Vr = Vref[:, :K]
        sub = np.linalg.norm(Vr - V @ (V.T @ Vr))
        if not sub < 1e-7:
            bad.append(f"invariant subspace: {sub:.3g}")
    return bad, dict(values=float(verr.max()), orth=float(orth), resid=float(resid), subspace=None if sub is None else float(sub))


def run_case(L, name, G, w, Vref, K, lam1=1.0, dl=(0, 0), may_fall_back=False, default_spectrum=False):
    """plan, two solves, bounds, accuracy; asserts at the end with every finding of the case"""
    s = G.shape[0]
    ldg, ldv = s + dl[0], s + dl[1]
    p = E.plan(s, K)
    bad = []
    got_plan = device_plan(L, s, K)
    if got_plan != E.plan_ints(p):
        bad.append(f"flgp_dev_eig_plan says {got_plan}, the restatement {E.plan_ints(p)}")
    t0 = time.perf_counter()
    _, pl, info = solve(L, G, K, ldg, ldv)
    t1 = time.perf_counter()
    _, pl2, info2 = solve(L, G, K, ldg, ldv)
    eig, V = pl.read_values(), pl.read_vectors()
    bad += pl.damage()
    if not (np.array_equal(eig.view(np.int64), pl2.read_values().view(np.int64))
            and np.array_equal(V.view(np.int64), pl2.read_vectors().view(np.int64)) and info == info2):
        bad.append(f"the second solve differs from the first (info {info} / {info2})")
    fell_back = info["dense"] and not p["dense"]
    if info["dense"] != p["dense"] and not (fell_back and may_fall_back):
        bad.append(f"info['dense'] = {info['dense']}, the plan says {p['dense']}")
    if default_spectrum and not p["dense"] and not info["outer_iterations"] >= 3:
        bad.append(f"converged in {info['outer_iterations']} outer iterations: no late Rayleigh-Ritz step")
    if not bad or np.isfinite(eig).all() and np.isfinite(V).all():
        acc, fig = accuracy(G, w, Vref, K, lam1, eig, V)
        bad += acc
    else:
        fig = {}
    print(f"[eig-edges] {name} s={s} K={K} ld=+{dl[0]}/+{dl[1]} plan={got_plan} it={info['outer_iterations']} "
          f"gprods={info['g_products']} ns={info['newton_schulz_orths']} jac={info['jacobi_orths']} dense={info['dense']} "
          f"fallback={fell_back} first_solve={t1 - t0:.3f}s {fig}")
    assert not bad, f"{name} (s={s}, K={K}, ldg={ldg}, ldv={ldv}):\n  " + "\n  ".join(bad)
    return info


def default_problem(s, K):
    return E.problem("default", s, None, E.SEEDS.get((s, K)))


# ------------------------------------------------------------------------------------------------- the tables
@pytest.mark.parametrize("s,K", E.TRUNCATED_CASES, ids=lambda v: str(v))
def test_truncated(stages, s, K):
    """b = 32 ... 1104: the three Jacobi kernels at their boundaries, padded block columns, the three refinement routes"""
    run_case(stages.L, "truncated", *default_problem(s, K), K, default_spectrum=True)


@pytest.mark.parametrize("s,K", E.DENSE_CASES, ids=lambda v: str(v))
def test_dense(stages, s, K):
    """the full decomposition on each of the four Jacobi kernels, at their boundaries"""
    run_case(stages.L, "dense", *default_problem(s, K), K, default_spectrum=True)


@pytest.mark.parametrize("s,K", E.BLOCKSPARSE_CASES + [E.BLOCKSPARSE_TWIN], ids=lambda v: str(v))
def test_blocksparse(stages, s, K):
    """the Gram matrix of a sparse ring graph, anchors permuted: the block-sparse products from s = 1536 on (the set-up, asked
    through flgp_dev_bsg_apply, says it would take that route and keeps blocks), the dense-G products one below"""
    L = stages.L
    G, w, Vref = E.problem("bs", s)
    if (s, K) != E.BLOCKSPARSE_TWIN:
        b = E.plan(s, K)["b"]
        wb = L.flgp_dev_bsg_workspace(s, b)
        work = torch.empty((wb // 8 + 1,), dtype=torch.float64, device=DEV)
        X = torch.ones((b, s), dtype=torch.float64, device=DEV)
        out = torch.empty((b, s), dtype=torch.float64, device=DEV)
        dG = torch.from_numpy(G.copy()).to(DEV)             # (the cached matrix is read-only)
        info = (ctypes.c_int * 6)()
        _lib.check(L.flgp_dev_bsg_apply(stream(), dG.data_ptr(), s, s, X.data_ptr(), b, 1.0, 0.0, None, out.data_ptr(),
                                        work.data_ptr(), wb, ctypes.addressof(info)))
        torch.cuda.synchronize()
        assert info[0] == 1, "the solver would not have chosen the block-sparse products for this matrix"
        assert info[2] > 0
    run_case(L, "block-sparse", G, w, Vref, K, lam1=w[0])


@pytest.mark.parametrize("dl", E.STRIDES, ids=lambda v: f"ldg+{v[0]}-ldv+{v[1]}")
@pytest.mark.parametrize("kind,s,K", E.STRIDE_CASES, ids=lambda v: str(v))
def test_strides(stages, kind, s, K, dl):
    """ldg != s and ldv != s on the dense route, the truncated route with rot.hip's and with the general products, and the
    block-sparse route.  A stride enters addresses only: the a-priori bounds, the filter degrees and the stop are functions
    of G's entries, so the solve takes the outer iterations, products and orthonormalisations of the same matrix at
    ldg = ldv = s.  (A kernel that reads G with the wrong stride need not fail the accuracy bars: apriori_bounds_kernel's
    maximum drops a column sum that is NaN, and bounds that are merely wrong only change the first filter.)"""
    G, w, Vref = E.problem("bs", s) if kind == "bs" else default_problem(s, K)
    info = run_case(stages.L, "strides", G, w, Vref, K, lam1=w[0], dl=dl, default_spectrum=kind == "default")
    _, _, tight = solve(stages.L, G, K, s, s)
    assert info == tight, f"ldg = s + {dl[0]}, ldv = s + {dl[1]}: {info}; ldg = ldv = s: {tight}"


@pytest.mark.parametrize("kind", E.SPECIAL_KINDS)
@pytest.mark.parametrize("s,K", E.SPECIAL_CASES, ids=lambda v: str(v))
def test_special_spectra(stages, s, K, kind):
    """a rank below b (below K + guard), a five-fold eigenvalue straddling position K, and the default matrix times 2^-40
    and 2^40.  The wanted eigenvalues are all >= 0.2 lambda_1, so the relative bar applies as it stands.  A truncated solve
    may end in the full decomposition only on the first two."""
    G, w, Vref, scale = E.special_problem(kind, s, K)
    assert w[K - 1] >= 0.2 * w[0]
    run_case(stages.L, kind, G, w, Vref, K, lam1=scale, may_fall_back=kind in ("rank", "cluster"))


# ------------------------------------------------------------------------------------------------- tol
@pytest.mark.parametrize("kind,s,K", E.TOL_CASES, ids=lambda v: str(v))
def test_tol(stages, kind, s, K):
    """the stop rule is rmax <= tol theta_1, measured on the device: every wanted pair's residual 2-norm is <= 2 tol lambda_1
    (the factor 2 covers the rounding of the rotated G A and of the host recomputation, both <= 1e-12 lambda_1),
    |theta_j - lambda_j| <= 2 sqrt(K) tol lambda_1, and a looser tol never costs more products"""
    L = stages.L
    G, w, Vref = E.problem("bs", s) if kind == "bs" else default_problem(s, K)
    lam1 = w[0]
    _, _, base = solve(L, G, K, s, s)
    bad = []
    for tol in E.TOLS:
        _, pl, info = solve(L, G, K, s, s, tol=tol)
        eig, V = pl.read_values(), pl.read_vectors()
        bad += pl.damage()
        rn = np.linalg.norm(G @ V - V * eig, axis=0)
        verr = np.abs(eig - w[:K]).max()
        print(f"[eig-edges] tol={tol:g} {kind} s={s} K={K} it={info['outer_iterations']} gprods={info['g_products']} "
              f"(default {base['g_products']}) max residual norm {rn.max():.3g} max value error {verr:.3g}")
        if not rn.max() <= 2.0 * tol * lam1:
            bad.append(f"tol {tol:g}: residual norm {rn.max():.3g}")
        if not verr <= 2.0 * np.sqrt(K) * tol * lam1:
            bad.append(f"tol {tol:g}: value error {verr:.3g}")
        if not info["g_products"] <= base["g_products"]:
            bad.append(f"tol {tol:g}: {info['g_products']} products, the default tolerance {base['g_products']}")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------- a refusal
def test_zero_matrix_is_refused_and_the_next_solve_is_right(stages):
    L = stages.L
    s, K = E.REFUSAL_CASE
    rc, pl, _ = solve(L, np.zeros((s, s)), K, s, s, check=False)
    assert rc == -1 and "zero or not finite" in L.flgp_last_error().decode()          # FLGP_ERR_INVALID
    assert (pl.work[pl.work_bytes // 8:].cpu().numpy() == E.CANARY_BITS).all()
    run_case(L, "after the refusal", *default_problem(s, K), K, default_spectrum=True)
