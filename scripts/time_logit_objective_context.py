"""Timing of the logit training context (flgp_logit_batch_*, LogitObjectiveBatch) against the entries it
stands beside, on ten synthetic resident pairs (n = 1e5 each: after the gather only the m rows matter), K = 200 and ten
one-vs-rest indicator columns, at m = 1000 and m = 1e4:

  (a) one hundred problems (ten pairs x ten classes): route A = ten logit_objective_batch calls, one per pair, against one
      evaluation of a context on all hundred;
  (b) one pair, ten problems: route A = the batch entry, against one evaluation of a context on that pair;
  (c) one problem: route A = the single entry, against one evaluation of a context of one; create and free are recorded too.

Wall clock around the Python call, same process, the two routes alternating, best of --reps after one warm-up of each.  The
gate is taken from the run itself: with route A's spread = max - min of its reps, (a) passes if the gain (A - context)
exceeds the spread, (b) and (c) pass if the context is not slower than route A by more than the spread.  Per row also the
device time of one batched iteration of the context's evaluation and its scopes ("logit_lr_batch_iter": == max(iters)
when the evaluation was one chunk), and whether every value and count equals route A's bit for bit.  Writes one JSON object
to --out.

Usage: python scripts/time_logit_objective_context.py [--reps 5] [--out profiles/logit_objective_context_timing.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logit_objective_context_timing.json"))
    args = ap.parse_args()
    torch.cuda.init()       # torch's HIP runtime opens the device before libflgp_hip.so does
    n, K, J, P = args.n, 200, 10, args.pairs
    rng = np.random.default_rng(0)
    rps = []
    for _ in range(P):
        values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
        V = np.asfortranarray(rng.standard_normal((n, K)))
        rps.append(api.ResidentEigenPair.from_host(api.EigenPair(values, V)))
        del V
    sigma = 1e-3
    L = _lib.lib()
    res = {"shape": dict(n=n, K=K, classes=J, pairs=P), "sigma": sigma, "reps": args.reps, "max_parallel": 0, "rows": []}

    for m in (1000, 10_000):
        idx = np.arange(m)
        labels = rng.integers(0, J, m)
        Y = np.asfortranarray((labels[:, None] == np.arange(J)[None, :]).astype(np.float64))
        cols = np.arange(J, dtype=np.int32)
        tgrid = np.linspace(1.0, 8.0, J)

        def batch_calls(pairs, col, ts):
            """route A of (a) and (b): one batch call per pair"""
            out = [rp.logit_objective_batch(ts, K, idx, Y, col=col, sigma=sigma, max_parallel=0, return_iters=True) for rp in pairs]
            return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])

        def single_call(pairs, col, ts):
            """route A of (c)"""
            v, i = pairs[0].logit_objective(float(ts[0]), K, idx, Y[:, int(col[0])], sigma=sigma, return_iters=True)
            return np.array([v]), np.array([i], dtype=np.int32)

        cases = [("a", rps, cols, tgrid, batch_calls), ("b", rps[:1], cols, tgrid, batch_calls),
                 ("c", rps[:1], cols[:1], np.array([4.0]), single_call)]
        for name, pairs, col, ts, route_a in cases:
            listed = [rp for rp in pairs for _ in col]                       # problem p J + j: class j on pair p
            pcol = np.tile(col, len(pairs)); pts = np.tile(ts, len(pairs))

            def make():
                return api.LogitObjectiveBatch(listed, K, idx, Y, col=pcol, sigma=sigma, max_parallel=0)
            t0 = time.perf_counter(); ctx = make(); t_create = time.perf_counter() - t0
            ref = route_a(pairs, col, ts); got = ctx(pts, return_iters=True)    # the warm-up of both routes
            ta, tb = [], []
            for _ in range(args.reps):                                        # alternating
                t0 = time.perf_counter(); ref = route_a(pairs, col, ts); ta.append(time.perf_counter() - t0)
                t0 = time.perf_counter(); got = ctx(pts, return_iters=True); tb.append(time.perf_counter() - t0)
            L.flgp_prof_reset(); L.flgp_prof_enable(2)
            ctx(pts)
            torch.cuda.synchronize(); L.flgp_prof_enable(0)
            cnt, ms = prof("logit_lr_batch_iter")
            L.flgp_prof_reset()
            t0 = time.perf_counter(); ctx.free(); t_free = time.perf_counter() - t0
            tc, tf = [], []
            for _ in range(args.reps):                                        # create and free, warm
                t0 = time.perf_counter(); c2 = make(); tc.append(time.perf_counter() - t0)
                t0 = time.perf_counter(); c2.free(); tf.append(time.perf_counter() - t0)
            a, b, spread = min(ta) * 1e3, min(tb) * 1e3, (max(ta) - min(ta)) * 1e3
            row = {"comparison": name, "m": m, "B": len(listed), "P": len(pairs), "chunk": ctx.chunk,
                   "route_a": "single entry" if name == "c" else "%d logit_objective_batch call(s)" % len(pairs),
                   "route_a_ms": a, "route_a_median_ms": float(np.median(ta)) * 1e3, "route_a_spread_ms": spread,
                   "context_ms": b, "context_median_ms": float(np.median(tb)) * 1e3,
                   "context_spread_ms": (max(tb) - min(tb)) * 1e3, "ratio": a / b, "gain_ms": a - b,
                   "gate": "gain > spread" if name == "a" else "context - route A <= spread",
                   "gate_pass": bool(a - b > spread) if name == "a" else bool(b - a <= spread),
                   "first_create_ms": t_create * 1e3, "first_free_ms": t_free * 1e3, "create_ms": min(tc) * 1e3,
                   "free_ms": min(tf) * 1e3, "iters": got[1].tolist(), "sum_iters": int(got[1].sum()),
                   "max_iters": int(got[1].max()), "context_iter_scopes": cnt, "context_iter_device_ms": ms / max(cnt, 1),
                   "bits_equal": bool(ref[0].tobytes() == got[0].tobytes() and np.array_equal(ref[1], got[1]))}
            res["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    for rp in rps:
        rp.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
