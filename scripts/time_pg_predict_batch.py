"""Timing of the batched Polya-Gamma prediction (flgp_eigenpair_pg_predict_batch) against the routes it
stands beside, on a synthetic resident pair with n = 1e6, K = 200, m_new = n - m new rows, N_sample = 100 and ten classes:

  * route A: flgp_eigenpair_pg_predict_multiclass for B = 10 (when profiles/pg_predict_batch_timing.json was taken: the ten
    chains one after another on one stream; it is the batch of J now), B calls of flgp_eigenpair_pg_predict
    otherwise;
  * route under test: one batch call (max_parallel = 0);
  * m = 1000 and 1e4 with B = 1, 10, 40 (the Woodbury sweep), and m = 200 = K with B = 10 (the m x m route's workers).

Same process, the two routes alternating, best of --reps after one warm-up of each.  Per row: both times, route A's
run-to-run spread (max - min over its reps), the device time of one batched sweep and the number of "pg_batch_sweep"
scopes of one call, and whether pi of the batch equals route A's bit for bit.  Writes one JSON object to --out.

--trace B: no timing; ONE batch call of B chains at --trace-m with --trace-ns sweeps, for a kernel trace of the run: the
launch count of a sweep is the difference of two traces' kernel counts over the difference of their --trace-ns.

Usage: python scripts/time_pg_predict_batch.py [--reps 5] [--out profiles/pg_predict_batch_timing.json]
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


def chains(B):
    """(col, ts): B = 1: class 0 at t = 4; B = 10: the ten classes at one t each; B = 40: ten classes x four t."""
    if B == 1:
        return np.zeros(1, dtype=np.int32), np.array([4.0])
    if B == 10:
        return np.arange(10, dtype=np.int32), np.linspace(2.0, 6.0, 10)
    return np.repeat(np.arange(10, dtype=np.int32), 4), np.tile(np.array([2.0, 3.0, 4.0, 6.0]), 10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pg_predict_batch_timing.json"))
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--trace-m", type=int, default=1000)
    ap.add_argument("--trace-ns", type=int, default=2)
    args = ap.parse_args()
    torch.cuda.init()       # torch's HIP runtime opens the device before libflgp_hip.so does
    n, K, ns, seed = args.n, 200, 100, 1
    rng = np.random.default_rng(0)
    values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
    V = np.asfortranarray(rng.standard_normal((n, K)) / np.sqrt(K))
    rp = api.ResidentEigenPair.from_host(api.EigenPair(values, V))
    del V
    sigma = 1e-3
    L = _lib.lib()

    def routes(m):
        idx0 = np.arange(m); idx1 = np.arange(m, n)
        labels = rng.integers(0, 10, m).astype(np.float64)
        Y = np.asfortranarray((labels[:, None] == np.arange(10)[None, :]).astype(np.float64))

        def existing(col, ts, nsamp=ns):
            if len(ts) == 10:          # chain j is class j with seed + j: the multiclass entry's own layout
                return rp.predict_logit_mult_gp_cpp(idx0, idx1, K, ts, labels, sigma, N_sample=nsamp, seed=seed, output_probs=True)[1]
            return np.stack([rp.test_pgbinary(idx0, idx1, K, float(t), Y[:, int(c)], sigma, 0.0, N_sample=nsamp, output_pi=True,
                                              seed=seed + b)["pi_pred"] for b, (c, t) in enumerate(zip(col, ts))], axis=1)

        def batch(col, ts, nsamp=ns):
            return rp.test_pgbinary_batch(idx0, idx1, K, ts, Y, sigma, 0.0, col=col, seed=seed, N_sample=nsamp, max_parallel=0,
                                          output_pi=True)["pi_pred"]
        return existing, batch

    if args.trace:
        _, batch = routes(args.trace_m)
        col, ts = chains(args.trace)
        batch(col, ts, args.trace_ns)
        rp.free()
        print(json.dumps({"trace_B": args.trace, "m": args.trace_m, "calls": 1, "N_sample": args.trace_ns}))
        return

    res = {"shape": dict(n=n, K=K, classes=10, N_sample=ns), "sigma": sigma, "reps": args.reps, "max_parallel": 0, "rows": []}
    for m, Bs in ((1000, (1, 10, 40)), (10_000, (1, 10, 40)), (200, (10,))):
        existing, batch = routes(m)
        for B in Bs:
            col, ts = chains(B)
            ref = existing(col, ts, 2); got = batch(col, ts, 2)                # the warm-up of both routes
            ta, tb = [], []
            for _ in range(args.reps):                                         # alternating
                t0 = time.perf_counter(); ref = existing(col, ts); ta.append(time.perf_counter() - t0)
                t0 = time.perf_counter(); got = batch(col, ts); tb.append(time.perf_counter() - t0)
            L.flgp_prof_reset(); L.flgp_prof_enable(2)
            batch(col, ts)
            torch.cuda.synchronize(); L.flgp_prof_enable(0)
            cnt, ms = prof("pg_batch_sweep")
            L.flgp_prof_reset()
            a, b = min(ta) * 1e3, min(tb) * 1e3
            row = {"m": m, "B": B, "route": "woodbury chunk" if m > K else "m x m workers",
                   "route_a": "pg_predict_multiclass" if B == 10 else "%d calls of pg_predict" % B,
                   "route_a_ms": a, "route_a_median_ms": float(np.median(ta)) * 1e3, "route_a_spread_ms": (max(ta) - min(ta)) * 1e3,
                   "batch_ms": b, "batch_median_ms": float(np.median(tb)) * 1e3, "batch_spread_ms": (max(tb) - min(tb)) * 1e3,
                   "speedup": a / b, "batch_sweep_scopes": cnt, "batch_sweep_device_ms": ms / max(cnt, 1),
                   "bits_equal": bool(np.array_equal(ref, got))}
            res["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    rp.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
