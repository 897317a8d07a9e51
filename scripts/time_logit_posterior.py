"""Timing of the logit posterior on the resident pair (flgp_eigenpair_logit_posterior) against the dense
entry (flgp_eigenpair_posterior_classification, the only route before it), on a synthetic resident pair with n = 1e6,
K = 200, t = 4, sigma11 = sigma22 = 1e-3 and m_new = n - m.  Prints one JSON object and writes it to
profiles/logit_posterior_timing.json:

  * for m = 1000, 1e4 and 1e5: the whole call of the new entry (wall clock around the C call, so the upload of Y and the
    two m_new-vectors coming down are in it), its Newton iterations, the device time of one iteration and of the
    predictive step alone (flgp_prof: HIP events on the entry's stream), and whether the loop met |f - f_new|_1 < tol
    before max_iter;
  * for m = 1000 and 1e4: the same figures of the dense entry; its predictive step is gemm_nn + gpr_rowquad.

Best of --reps after a warm-up, the two entries alternating in one process.

--single: the three entries alone, wall clock, at the rows of single_rows(); --compare PARENT_LIB: that under the parent
commit's library and this tree's in alternating fresh processes, with the gate of compare()
(profiles/logit_posterior_fold_timing.json).

Usage: python scripts/time_logit_posterior.py [--reps 5]
       python scripts/time_logit_posterior.py --compare /path/to/parent/libflgp_hip.so --out profiles/logit_posterior_fold_timing.json
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from flgp_amd import _lib, api  # noqa: E402


def prof(name):
    c = ctypes.c_int(); ms = ctypes.c_double(); w = ctypes.c_double()
    _lib.lib().flgp_prof_query(name.encode(), ctypes.addressof(c), ctypes.addressof(ms), ctypes.addressof(w))
    return c.value, ms.value


def measure(fn, reps, iter_name, predict_name):
    """Best wall time of fn over reps plain calls, then best per-iteration and predictive device times over reps profiled calls."""
    L = _lib.lib()
    fn()                                                        # warm-up
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter(); out = fn(); wall.append(time.perf_counter() - t0)
    it_ms, pr_ms = [], []
    for _ in range(reps):
        L.flgp_prof_reset(); L.flgp_prof_enable(2)
        fn()
        torch.cuda.synchronize(); L.flgp_prof_enable(0)
        c, ms = prof(iter_name); it_ms.append(ms / max(c, 1))
        c, ms = prof(predict_name); pr_ms.append(ms / max(c, 1))
    L.flgp_prof_reset()
    return dict(call_ms=min(wall) * 1e3, call_median_ms=float(np.median(wall)) * 1e3, iter_device_ms=min(it_ms),
                predict_device_ms=min(pr_ms)), out


def single_rows(reps):
    """--single: the binary, the one-vs-rest and the batch entry alone at n = 1e6, K = 200, m_new = n - m (wall clock around
    the Python call, best of `reps` after a warm-up).  {row: ms}"""
    n, K, J, s11, s22, tol = 1_000_000, 200, 10, 0.0, 1e-3, 1e-5
    rng = np.random.default_rng(0)
    values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
    V = np.asfortranarray(rng.standard_normal((n, K)))
    rp = api.ResidentEigenPair.from_host(api.EigenPair(values, V))
    del V
    ts = np.linspace(1.0, 8.0, J)
    out = {}

    def row(name, fn):
        fn()
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); wall.append(time.perf_counter() - t0)
        out[name] = min(wall) * 1e3

    for m in (1000, 10_000, 100_000, 200):
        idx0 = np.arange(m); idx1 = np.arange(m, n)
        Y = (rng.uniform(size=m) < 0.3).astype(np.float64)
        row(f"binary m={m}" + (" dense" if m <= K else ""), lambda: rp.logit_posterior(idx0, idx1, K, 4.0, Y, 1e-3, 1e-3, tol))
    for m in (1000, 10_000):
        idx0 = np.arange(m); idx1 = np.arange(m, n)
        labels = rng.permutation(np.arange(m) % J).astype(np.float64)         # balanced labels
        target = rng.integers(0, J, n - m).astype(np.float64); target[0] = J - 1
        row(f"multiclass J={J} m={m} default", lambda: rp.logit_posterior_multiclass(idx0, idx1, K, ts, labels, s22, s11, tol))
        row(f"multiclass J={J} m={m} max_parallel=J",
            lambda: rp.logit_posterior_multiclass(idx0, idx1, K, ts, labels, s22, s11, tol, max_parallel=J))
        row(f"multiclass J={J} m={m} nll only",
            lambda: rp.logit_posterior_multiclass(idx0, idx1, K, ts, labels, s22, s11, tol, target=target, n_samples=100, seed=1,
                                                  return_posterior=False))
        if m == 10_000:
            ind = np.asfortranarray((labels[:, None] == np.arange(J)[None, :]).astype(np.float64))
            row(f"batch B={J} m={m}", lambda: rp.logit_posterior_batch(idx0, idx1, K, ts, ind, sigma11=s11, sigma22=s22, tol=tol))
    rp.free()
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
    res = {"shape": dict(n=1_000_000, K=200), "rounds": rounds, "reps": reps, "rows": rows}
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--single", action="store_true", help="time the entries alone (see single_rows)")
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
    n, K, t, sigma, tol = 1_000_000, 200, 4.0, 1e-3, 1e-5
    rng = np.random.default_rng(0)
    values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
    V = np.asfortranarray(rng.standard_normal((n, K)))
    rp = api.ResidentEigenPair.from_host(api.EigenPair(values, V))
    res = {"shape": dict(n=n, K=K, t=t, sigma=sigma, tol=tol, max_iter=args.max_iter), "reps": args.reps, "rows": []}
    for m in (1000, 10_000, 100_000):
        idx0 = np.arange(m); idx1 = np.arange(m, n)
        Y = (rng.uniform(size=m) < 0.3).astype(np.float64)
        row = dict(m=m, m_new=n - m)

        def new():
            return rp.logit_posterior(idx0, idx1, K, t, Y, sigma, sigma, tol, args.max_iter, return_iters=True)

        def old():
            return rp.posterior_distribution_classification(idx0, idx1, K, t, Y, sigma, sigma, tol, args.max_iter)

        # alternate the routes: one block of each, new first, where the dense route exists at a bearable cost
        figs, (post, iters) = measure(new, args.reps, "logit_ws_batch_iter", "gpc_predict_rows_multi")
        row["logit_posterior"] = dict(figs, iterations=iters, converged=bool(iters < args.max_iter),
                                      min_cov=float(post["cov"].min()))
        if m <= 10_000:
            figs, dense = measure(old, args.reps, "logit_la_newton_iter", "posterior_dense_predict")
            row["posterior_classification"] = dict(figs, max_abs_dmean=float(np.abs(dense["mean"] - post["mean"]).max()),
                                                   max_abs_mean=float(np.abs(dense["mean"]).max()),
                                                   max_abs_dcov=float(np.abs(dense["cov"] - post["cov"]).max()))
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    rp.free()
    out = os.path.join(ROOT, "profiles", "logit_posterior_timing.json")
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
