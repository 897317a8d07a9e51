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

Usage: python scripts/time_logit_posterior.py [--reps 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=100)
    args = ap.parse_args()
    torch.cuda.init()       # torch's HIP runtime opens the device before libflgp_hip.so does
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
        figs, (post, iters) = measure(new, args.reps, "logit_ws_newton_iter", "gpc_predict_rows")
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
