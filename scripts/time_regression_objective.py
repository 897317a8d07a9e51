"""Timing of the regression training objectives on the resident pair at the two full-size shapes:
Woodbury n = 1e6, K = 200, m = 1000 and direct n = 1e5, K = 2000, m = 1000, on synthetic pairs.  Prints one JSON object
with, per shape and noise model:

  * value_ms / value_grad_ms: one evaluation without / with the gradient (best of --reps after a warm-up, and the median);
  * stages_ms: flgp_prof device times of one profiled evaluation with the gradient;
  * host_route_ms: the route the adapters take today -- H (direct) or the V rows (Woodbury) down, then the reference's
    algebra in numpy / LAPACK (dense C^-1, U, G; Q^-1 and the per-row terms);

and, at m = 1000, the triangular inverse alone (its flgp_prof time inside the direct evaluation) against chol_trsv with m
right-hand sides on the identity (flgp_dev_chol_solve, mode 1), the route the inverse replaces.

--single: the single entry alone, wall clock, at the rows of single_rows(); --compare PARENT_LIB: that under the parent
commit's library and this tree's in alternating fresh processes, with the gate of compare()
(profiles/regression_objective_single_timing.json).

Usage: python scripts/time_regression_objective.py [--reps 5]
       python scripts/time_regression_objective.py --compare /path/to/parent/libflgp_hip.so --out profiles/regression_objective_single_timing.json
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import scipy.linalg as sl

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from flgp_amd import _lib, api  # noqa: E402

STAGES = ("hk_panel_kernel", "chol_blocked", "tri_inverse", "gemm_f64_kernel")


def prof(name):
    c = ctypes.c_int(); ms = ctypes.c_double(); w = ctypes.c_double()
    _lib.lib().flgp_prof_query(name.encode(), ctypes.addressof(c), ctypes.addressof(ms), ctypes.addressof(w))
    return c.value, ms.value


def best(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); out = fn(); ts.append(time.perf_counter() - t0)
    return min(ts), float(np.median(ts)), out


def host_direct(rp, values, K, idx, Y, x, sigma, noise):
    """src/train.cpp:362-387 / 469-489 after H comes down (and the V rows, for grad_t)"""
    m, q = Y.shape
    t = x[0]
    C = rp.HK_from_spectrum_cpp(K, t, idx, idx) + sigma * np.eye(m)
    C += np.diag(x[1:]) if noise == "different" else x[1] * np.eye(m)
    V = rp.VC(K, idx, np.eye(K))
    L = sl.cholesky(C, lower=True)
    alpha = sl.cho_solve((L, True), Y)
    Cinv = sl.cho_solve((L, True), np.eye(m))
    U = alpha @ alpha.T / q - Cinv
    lam = 1.0 - values[:K]
    G = (V * (-lam * np.exp(-t * lam))) @ V.T
    g0 = -0.5 * (U * G.T).sum()
    g1 = -0.5 * np.diag(U) if noise == "different" else -0.5 * np.trace(U)
    return 0.5 * (Y * alpha).sum() / q + np.log(np.diag(L) + 1e-9).sum(), g0, g1


def host_woodbury(rp, values, K, idx, Y, x, sigma, noise):
    """src/train.cpp:395-433 / 492-552 after the V rows come down"""
    m, q = Y.shape
    t = x[0]
    V = rp.VC(K, idx, np.eye(K))
    lam = 1.0 - values[:K]
    Ls = np.exp(-0.5 * t * lam)
    A = -lam * np.exp(-t * lam)
    zi = 1.0 / (x[1:] + sigma) if noise == "different" else np.full(m, 1.0 / (x[1] + sigma))
    M = V.T @ (zi[:, None] * V)
    Q = Ls[:, None] * M * Ls[None, :] + np.eye(K)
    LQ = sl.cholesky(Q, lower=True)
    alpha = zi[:, None] * (Y - V @ (Ls[:, None] * sl.cho_solve((LQ, True), Ls[:, None] * (V.T @ (zi[:, None] * Y)))))
    Qinv = sl.cho_solve((LQ, True), np.eye(K))
    Vta = V.T @ alpha
    g0 = -0.5 * (Vta * (A[:, None] * Vta)).sum() / q + 0.5 * np.trace(A[:, None] * M)
    g0 += -0.5 * ((Qinv @ (Ls[:, None] * M)) * (A[:, None] * M * Ls[None, :]).T).sum()
    tmp = zi[:, None] * V * Ls[None, :]
    gi = -0.5 * (alpha * alpha).sum(1) / q + 0.5 * (zi - ((tmp @ Qinv) * tmp).sum(1))
    return 0.5 * (Y * alpha).sum() / q + np.log(np.diag(LQ)).sum(), g0, gi


def shape_case(n, K, m, reps, seed):
    rng = np.random.default_rng(seed)
    values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
    V = np.asfortranarray(rng.standard_normal((n, K)))
    rp = api.ResidentEigenPair.from_host(api.EigenPair(values, V))
    del V
    idx = rng.choice(n, m, replace=False)
    Y = rng.standard_normal((m, 1))
    sigma = 1e-5
    L = _lib.lib()
    out = {"shape": dict(n=n, K=K, m=m, branch="direct" if m <= K else "woodbury")}
    for noise in ("same", "different"):
        x = np.r_[3.0, 0.2] if noise == "same" else np.r_[3.0, rng.uniform(0.05, 0.4, m)]
        f = lambda g: rp.regression_objective(x, K, idx, Y, sigma=sigma, noise=noise, grad=g)  # noqa: E731
        f(True); f(False)                                                                     # warm-up
        v_min, v_med, _ = best(lambda: f(False), reps)
        g_min, g_med, _ = best(lambda: f(True), reps)
        L.flgp_prof_reset(); L.flgp_prof_enable(2)
        f(True)
        torch.cuda.synchronize(); L.flgp_prof_enable(0)
        stages = {}
        for s in STAGES:
            c, ms = prof(s)
            if c:
                stages[s] = dict(calls=c, ms=ms)
        host = host_direct if m <= K else host_woodbury
        h_min, h_med, _ = best(lambda: host(rp, values, K, idx, Y, x, sigma, noise), max(2, reps // 2))
        out[noise] = dict(value_ms=v_min * 1e3, value_median_ms=v_med * 1e3, value_grad_ms=g_min * 1e3,
                          value_grad_median_ms=g_med * 1e3, stages_ms=stages, host_route_ms=h_min * 1e3,
                          host_route_median_ms=h_med * 1e3, speedup=h_min / g_min)
    rp.free()
    return out


def inverse_vs_trsv(m, reps, tri_ms):
    """chol_trsv with m right-hand sides (mode 1 on the identity) gives L^-1 as well"""
    rng = np.random.default_rng(1)
    x = rng.uniform(-3, 3, size=(m, 2))
    C = 4.0 * np.exp(-0.5 * ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)) + np.eye(m)
    Lm = torch.tensor(C.T.copy(), device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    L = _lib.lib()
    _lib.check(L.flgp_dev_cholesky(None, Lm.data_ptr(), m, 0, flag.data_ptr()))
    eye = torch.eye(m, dtype=torch.float64, device="cuda")
    times = []
    for r in range(reps + 1):
        B = eye.clone()
        torch.cuda.synchronize()
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(L.flgp_dev_chol_solve(None, Lm.data_ptr(), m, B.data_ptr(), m, 1, flag.data_ptr()))
        e1.record(); torch.cuda.synchronize()
        if r:
            times.append(e0.elapsed_time(e1))
    assert flag.item() == 0
    return dict(m=m, tri_inverse_ms=tri_ms, trsv_m_rhs_ms=min(times), trsv_m_rhs_median_ms=float(np.median(times)))


def single_rows(reps):
    """--single: the single entry alone at n = 1e6, K = 200, q = 1 (wall clock around the Python call, best of `reps` after a
    warm-up), and one eval of a B = 10 context at m = 1000 "same".  {row: ms}"""
    n, K, sigma = 1_000_000, 200, 1e-5
    rng = np.random.default_rng(0)
    V = np.asfortranarray(rng.standard_normal((n, K)))
    pairs = []
    for _ in range(10):     # ten pairs on the same vectors, values of their own
        pairs.append(api.ResidentEigenPair.from_host(api.EigenPair(np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy(), V)))
    del V
    rp = pairs[0]
    out = {}

    def row(name, m, noise, grad, kind="scattered"):
        idx = np.arange(5000, 5000 + m) if kind == "range" else rng.choice(n, m, replace=False)
        Y = rng.standard_normal((m, 1))
        x = np.r_[3.0, 0.2] if noise == "same" else np.r_[3.0, rng.uniform(0.05, 0.4, m)]
        f = lambda: rp.regression_objective(x, K, idx, Y, sigma=sigma, noise=noise, grad=grad)  # noqa: E731
        f()
        out[name] = best(f, reps)[0] * 1e3

    for m in (1000, 10_000):
        for noise in ("same", "different"):
            row(f"woodbury m={m} {noise} grad", m, noise, True)
    row("woodbury m=1000 same value", 1000, "same", False)
    row("woodbury m=100000 same grad range", 100_000, "same", True, kind="range")
    for noise in ("same", "different"):
        row(f"direct m=200 {noise} grad", 200, noise, True)
    row("direct m=200 same value", 200, "same", False)
    idx = rng.choice(n, 1000, replace=False)
    Y = rng.standard_normal((1000, 1))
    X = np.array([np.r_[rng.uniform(1.0, 6.0), rng.uniform(0.05, 0.4)] for _ in range(10)])
    ctx = api.RegressionObjectiveBatch(pairs, K, idx, Y, sigma=sigma, noise="same")
    ctx(X)
    out["batch B=10 m=1000 same grad"] = best(lambda: ctx(X), reps)[0] * 1e3
    ctx.free()
    for p in pairs:
        p.free()
    return out


def compare(parent_lib, rounds, reps, out_path):
    """--compare: --single under the library of the parent commit and under this tree's, alternating, each round a fresh
    process with its own time limit.  Gate per row: head's best <= parent's best + parent's spread (max - min of its rounds)."""
    import subprocess
    runs = {"parent": [], "head": []}
    for _ in range(rounds):
        for who, lib in (("parent", parent_lib), ("head", None)):
            cmd = [sys.executable, os.path.abspath(__file__), "--single", "--reps", str(reps)] + (["--lib", lib] if lib else [])
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=400, check=True)
            runs[who].append(json.loads(res.stdout.strip().splitlines()[-1]))
            print(who, runs[who][-1], file=sys.stderr, flush=True)
    rows = []
    for name in runs["parent"][0]:
        p = [r[name] for r in runs["parent"]]; h = [r[name] for r in runs["head"]]
        rows.append(dict(row=name, parent_rounds_ms=p, head_rounds_ms=h, parent_best_ms=min(p), parent_spread_ms=max(p) - min(p),
                         head_best_ms=min(h), within_gate=bool(min(h) <= min(p) + (max(p) - min(p)))))
    res = {"shape": dict(n=1_000_000, K=200, q=1), "rounds": rounds, "reps": reps, "rows": rows}
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--single", action="store_true", help="time the single entry alone (see single_rows)")
    ap.add_argument("--lib", default=None, help="with --single: another build of libflgp_hip.so")
    ap.add_argument("--compare", default=None, metavar="PARENT_LIB", help="--single under PARENT_LIB and this tree's library")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.compare:
        return compare(args.compare, args.rounds, args.reps, args.out)
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    torch.cuda.init()       # torch's HIP runtime opens the device before libflgp_hip.so does
    if args.single:
        print(json.dumps(single_rows(args.reps)))
        return
    res = {"reps": args.reps}
    res["woodbury"] = shape_case(1_000_000, 200, 1000, args.reps, 0)
    res["direct"] = shape_case(100_000, 2000, 1000, args.reps, 1)
    tri = res["direct"]["same"]["stages_ms"].get("tri_inverse", {})
    res["inverse"] = inverse_vs_trsv(1000, args.reps, tri.get("ms"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
