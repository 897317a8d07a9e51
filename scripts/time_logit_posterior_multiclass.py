"""Timing of the one-vs-rest logit posterior in one call (flgp_eigenpair_logit_posterior_multiclass) against
what a caller could do before it: J calls of the binary entry (flgp_eigenpair_logit_posterior) and the host stacking.  A
synthetic resident pair with n = 1e6, K = 200; J = 10 classes with balanced labels, ten values of t from 1 to 8,
sigma11 = 0, sigma22 = 1e-3, m = 1000 and 1e4, m_new = n - m.  Prints one JSON object and writes it to
profiles/logit_posterior_multiclass_timing.json.  Per m:

  * A: the J binary calls with their columns stacked into two m_new x J arrays (wall clock).  Timed twice, as the first and
    the last block, so that A's own run-to-run spread is on record;
  * B: the new entry at max_parallel (classes per chunk) 1, 2, 4 and 8 (wall clock: the uploads and the two m_new x J arrays coming down are in it);
  * C: the _nll entry, score only (one double comes down);
  * the device time of the fused predictive pass of B at J classes per chunk against the sum of the J one-operand passes of
    A (both gpc_predict_rows_multi), by HIP events on the entries' streams (flgp_prof);
  * the wall time of the J modes alone at each chunk size: the new entry on one new row, where the pass is a single
    workgroup.

Best of --reps after a warm-up, the blocks alternating in one process in the order A, B1, B2, B4, B8, C, A.

Usage: python scripts/time_logit_posterior_multiclass.py [--reps 5] [--out FILE]
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

WORKERS = (1, 2, 4, 8)


def prof_sum(name):
    c = ctypes.c_int(); ms = ctypes.c_double(); w = ctypes.c_double()
    _lib.lib().flgp_prof_query(name.encode(), ctypes.addressof(c), ctypes.addressof(ms), ctypes.addressof(w))
    return c.value, ms.value


def wall(fn, reps):
    """best and median wall time (ms) of fn over reps calls after a warm-up, and the last result"""
    out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); out = fn(); ts.append(time.perf_counter() - t0)
    return dict(ms=min(ts) * 1e3, median_ms=float(np.median(ts)) * 1e3), out


def device_ms(fn, reps, name):
    """best over reps profiled calls of the summed device time of the scopes called `name`, and their count per call"""
    L = _lib.lib()
    best, count = None, 0
    for _ in range(reps):
        L.flgp_prof_reset(); L.flgp_prof_enable(2)
        fn()
        torch.cuda.synchronize(); L.flgp_prof_enable(0)
        count, ms = prof_sum(name)
        best = ms if best is None else min(best, ms)
    L.flgp_prof_reset()
    return best, count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logit_posterior_multiclass_timing.json"))
    args = ap.parse_args()
    torch.cuda.init()       # torch's HIP runtime opens the device before libflgp_hip.so does
    n, K, J, s11, s22, tol, max_iter = 1_000_000, 200, 10, 0.0, 1e-3, 1e-5, 100
    ts = np.linspace(1.0, 8.0, J)
    rng = np.random.default_rng(0)
    values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
    V = np.asfortranarray(rng.standard_normal((n, K)))
    rp = api.ResidentEigenPair.from_host(api.EigenPair(values, V))
    del V
    res = {"shape": dict(n=n, K=K, J=J, ts=ts.tolist(), sigma11=s11, sigma22=s22, tol=tol, max_iter=max_iter), "reps": args.reps,
           "rows": []}
    for m in (1000, 10_000):
        idx0 = np.arange(m); idx1 = np.arange(m, n)
        Y = rng.permutation(np.arange(m) % J).astype(np.float64)              # balanced labels
        target = rng.integers(0, J, n - m).astype(np.float64); target[0] = J - 1
        row = dict(m=m, m_new=n - m)

        def A():
            mean = np.zeros((n - m, J), order="F"); cov = np.zeros((n - m, J), order="F"); its = []
            for j in range(J):
                post, it = rp.logit_posterior(idx0, idx1, K, ts[j], (Y == j).astype(np.float64), s11, s22, tol, max_iter,
                                              return_iters=True)
                mean[:, j] = post["mean"]; cov[:, j] = post["cov"]; its.append(it)
            return mean, cov, its

        def B(workers, rows=idx1):
            return rp.logit_posterior_multiclass(idx0, rows, K, ts, Y, s22, s11, tol, max_iter, workers, return_iters=True)

        def C():
            return rp.logit_posterior_multiclass(idx0, idx1, K, ts, Y, s22, s11, tol, max_iter, 4, target=target, n_samples=100,
                                                 seed=1, return_posterior=False)

        a1, (mean, cov, its) = wall(A, args.reps)
        row["A_first"] = a1
        row["iterations"] = [int(i) for i in its]
        for w in WORKERS:
            row[f"B_{w}"], (post, its_b) = wall(lambda: B(w), args.reps)
            assert post["mean"].tobytes() == mean.tobytes() and post["cov"].tobytes() == cov.tobytes() and list(its_b) == list(its)
        row["C_score_only"], score = wall(C, args.reps)
        row["nll"] = score["nll"]
        row["A_last"], _ = wall(A, args.reps)
        row["A_spread_ms"] = abs(row["A_first"]["ms"] - row["A_last"]["ms"])
        row["A_ms"] = min(row["A_first"]["ms"], row["A_last"]["ms"])
        single, count = device_ms(A, args.reps, "gpc_predict_rows_multi")
        fused, _ = device_ms(lambda: B(J), args.reps, "gpc_predict_rows_multi")
        row["predict_device_ms"] = dict(J_single_passes=single, single_passes=count, fused_pass=fused)
        row["modes_wall_ms"] = {str(w): wall(lambda: B(w, idx1[:1]), args.reps)[0]["ms"] for w in WORKERS}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    rp.free()
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
