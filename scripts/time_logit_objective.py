"""Timing of the logit training objective (flgp_eigenpair_logit_objective) against the dense entry
flgp_eigenpair_logit_marginal_likelihood on a synthetic resident pair with n = 1e6, K = 200:

  * m = 200: the objective's dense route (m <= K), the same loop as the dense entry's;
  * m = 1000 (BASELINE configs[2]) and m = 1e4: both entries (the objective takes its low-rank route, m > K);
  * m = 1e5: the objective only (the dense one would need two 80 GB m x m matrices).

Each timing is the best (and median) of --reps calls after one warm-up, all of them kept (new_all_ms: their max - min is
the spread of the measurement), with the Newton iterations and the device time of one iteration from flgp_prof
("logit_lr_batch_iter" / "logit_la_newton_iter").  Prints one JSON object.

Usage: python scripts/time_logit_objective.py [--reps 5]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from flgp_amd import _lib, api  # noqa: E402


def prof(name):
    c = ctypes.c_int(); ms = ctypes.c_double(); w = ctypes.c_double()
    _lib.lib().flgp_prof_query(name.encode(), ctypes.addressof(c), ctypes.addressof(ms), ctypes.addressof(w))
    return c.value, ms.value


def best(fn, reps):
    fn()                                                       # warm-up
    ts = []
    out = None
    for _ in range(reps):
        t0 = time.perf_counter(); out = fn(); ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3, float(np.median(ts)) * 1e3, [t * 1e3 for t in ts], out


def iter_ms(fn, name):
    L = _lib.lib()
    L.flgp_prof_reset(); L.flgp_prof_enable(2)
    fn()
    torch.cuda.synchronize(); L.flgp_prof_enable(0)
    c, ms = prof(name)
    return ms / max(c, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    torch.cuda.init()       # torch's HIP runtime opens the device before libflgp_hip.so does
    n, K = 1_000_000, 200
    rng = np.random.default_rng(0)
    values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
    V = np.asfortranarray(rng.standard_normal((n, K)))
    rp = api.ResidentEigenPair.from_host(api.EigenPair(values, V))
    del V
    t, sigma = 4.0, 1e-3
    res = {"shape": dict(n=n, K=K), "t": t, "sigma": sigma, "reps": args.reps, "rows": []}
    for m, dense in ((1000, True), (10_000, True), (100_000, False), (200, True)):     # 200 last: the draws of Y stay
        idx = np.arange(m)
        Y = (rng.uniform(size=m) < 0.3).astype(np.float64)
        row = {"m": m}

        def new():
            return rp.logit_objective(t, K, idx, Y, sigma=sigma, approach="marginal", return_iters=True)
        row["new_ms"], row["new_median_ms"], row["new_all_ms"], (v, it) = best(new, args.reps)
        row["new_iters"], row["new_value"] = it, v
        row["new_iter_device_ms"] = iter_ms(new, "logit_lr_batch_iter" if m > K else "logit_la_newton_iter")
        if dense:
            def old():
                return rp.marginal_log_likelihood_logit_la(K, t, idx, Y, sigma=sigma, return_iters=True)
            row["dense_ms"], row["dense_median_ms"], _, (a, it_d) = best(old, args.reps)
            row["dense_iters"], row["dense_value"] = it_d, -a
            row["dense_iter_device_ms"] = iter_ms(old, "logit_la_newton_iter")
            row["speedup"] = row["dense_ms"] / row["new_ms"]
            row["value_diff"] = v + a
        res["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    rp.free()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
