"""Timing of the batched logit training objective (flgp_eigenpair_logit_objective_batch) against the route
it replaces, on a synthetic resident pair with n = 1e6, K = 200 and ten one-vs-rest classes:

  * route A: B single calls of flgp_eigenpair_logit_objective, one after another;
  * route B: one batch call (max_parallel = 0: one chunk where the memory allows);
  * m = 1000 and 1e4; B = 1, 10 (the ten classes at one t each) and 40 (ten classes x four t).

Same process, the two routes alternating, best of --reps after one warm-up of each.  Per row: both times, route A's
run-to-run spread (max - min over its reps), the device time of one batched iteration and the number of
"logit_lr_batch_iter" scopes of one call (== max(iters) when the whole batch was one chunk), and whether every value and
iteration count of the batch equals the single calls' bit for bit.  Writes one JSON object to --out.

--trace B: no timing; one warm-up and one batch call of B problems at --trace-m, for a kernel trace of the run (the launch
count of an iteration is the trace's count over the printed iteration count).

Usage: python scripts/time_logit_objective_batch.py [--reps 5] [--out profiles/logit_objective_batch_timing.json]
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


def problems(B, t0=4.0):
    """(col, ts): B = 1: class 0 at t0; B = 10: the ten classes at one t each; B = 40: ten classes x four t."""
    if B == 1:
        return np.zeros(1, dtype=np.int32), np.array([t0])
    if B == 10:
        return np.arange(10, dtype=np.int32), np.linspace(1.0, 8.0, 10)
    return np.repeat(np.arange(10, dtype=np.int32), 4), np.tile(np.array([0.5, 2.0, 4.0, 8.0]), 10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logit_objective_batch_timing.json"))
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--trace-m", type=int, default=1000)
    args = ap.parse_args()
    torch.cuda.init()       # torch's HIP runtime opens the device before libflgp_hip.so does
    n, K = args.n, 200
    rng = np.random.default_rng(0)
    values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
    V = np.asfortranarray(rng.standard_normal((n, K)))
    rp = api.ResidentEigenPair.from_host(api.EigenPair(values, V))
    del V
    sigma = 1e-3
    L = _lib.lib()

    def routes(m):
        idx = np.arange(m)
        labels = rng.integers(0, 10, m)
        Y = np.asfortranarray((labels[:, None] == np.arange(10)[None, :]).astype(np.float64))

        def single(col, ts):
            out = [rp.logit_objective(float(t), K, idx, Y[:, int(c)], sigma=sigma, return_iters=True) for c, t in zip(col, ts)]
            return np.array([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.int32)

        def batch(col, ts):
            return rp.logit_objective_batch(ts, K, idx, Y, col=col, sigma=sigma, max_parallel=0, return_iters=True)
        return single, batch

    if args.trace:
        single, batch = routes(args.trace_m)
        col, ts = problems(args.trace)
        batch(col, ts)
        _, its = batch(col, ts)
        rp.free()
        print(json.dumps({"trace_B": args.trace, "m": args.trace_m, "calls": 2, "iters": its.tolist(), "max_iters": int(its.max())}))
        return

    res = {"shape": dict(n=n, K=K, classes=10), "sigma": sigma, "reps": args.reps, "max_parallel": 0, "rows": []}
    for m in (1000, 10_000):
        single, batch = routes(m)
        for B in (1, 10, 40):
            col, ts = problems(B)
            ref = single(col, ts); got = batch(col, ts)                       # the warm-up of both routes
            ta, tb = [], []
            for _ in range(args.reps):                                         # alternating
                t0 = time.perf_counter(); ref = single(col, ts); ta.append(time.perf_counter() - t0)
                t0 = time.perf_counter(); got = batch(col, ts); tb.append(time.perf_counter() - t0)
            L.flgp_prof_reset(); L.flgp_prof_enable(2)
            batch(col, ts)
            torch.cuda.synchronize(); L.flgp_prof_enable(0)
            cnt, ms = prof("logit_lr_batch_iter")
            L.flgp_prof_reset()
            a, b = min(ta) * 1e3, min(tb) * 1e3
            one_chunk = cnt == int(got[1].max())
            row = {"m": m, "B": B, "single_calls_ms": a, "single_calls_median_ms": float(np.median(ta)) * 1e3,
                   "single_calls_spread_ms": (max(ta) - min(ta)) * 1e3, "batch_ms": b,
                   "batch_median_ms": float(np.median(tb)) * 1e3, "batch_spread_ms": (max(tb) - min(tb)) * 1e3,
                   "speedup": a / b, "iters": got[1].tolist(), "sum_iters": int(got[1].sum()), "max_iters": int(got[1].max()),
                   "batch_iter_scopes": cnt, "batch_iter_device_ms": ms / max(cnt, 1), "chunk_size": B if one_chunk else None,
                   "bits_equal": bool(ref[0].tobytes() == got[0].tobytes() and np.array_equal(ref[1], got[1]))}
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
