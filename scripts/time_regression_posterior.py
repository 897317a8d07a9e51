"""Timing of the regression posterior on the resident pair (flgp_eigenpair_regression_posterior) against
the three calls it replaces (predict_regression_cpp on the training rows and on the new rows,
posterior_covariance_regression), on a synthetic resident pair with n = 1e6, K = 200, q = 1, t = 4, noise = 0.1,
sigma = 1e-3 and m_new = n - m, for m = 1000 (BASELINE configs[2]), 1e4 and 1e5.  Host arrays in and out: wall clock around
the Python call.  --reps timed repetitions after a warm-up; the minimum and the median are kept.

The three existing calls are timed from whatever library the process loads: --lib PATH loads another build of
libflgp_hip.so (the parent commit's), --existing-only skips the new entry (which that build does not have) and --out
names the JSON.  A second run on this tree's library with --parent-json that file puts both into
profiles/regression_posterior_timing.json, with the per-launch table (flgp_prof: HIP events on the entry's stream) of
one profiled call of the new entry.

Usage: python scripts/time_regression_posterior.py --lib parent/libflgp_hip.so --existing-only --out parent.json
       python scripts/time_regression_posterior.py --parent-json parent.json
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

NEW = "flgp_eigenpair_regression_posterior"


def timed(fn, reps):
    fn()                                                        # warm-up
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter(); out = fn(); wall.append(time.perf_counter() - t0)
    return dict(call_ms=min(wall) * 1e3, call_median_ms=float(np.median(wall)) * 1e3), out


def prof_table(fn):
    """name -> (launch scopes, device ms) of one profiled call"""
    L = _lib.lib()
    L.flgp_prof_reset(); L.flgp_prof_enable(2)
    fn()
    torch.cuda.synchronize(); L.flgp_prof_enable(0)
    buf = ctypes.create_string_buffer(1 << 16)
    L.flgp_prof_names(ctypes.addressof(buf), len(buf))
    table = {}
    for name in buf.value.decode().split():
        c = ctypes.c_int(); ms = ctypes.c_double(); w = ctypes.c_double()
        L.flgp_prof_query(name.encode(), ctypes.addressof(c), ctypes.addressof(ms), ctypes.addressof(w))
        if c.value:
            table[name] = dict(count=c.value, device_ms=ms.value)
    L.flgp_prof_reset()
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--lib", help="another build of libflgp_hip.so to load")
    ap.add_argument("--existing-only", action="store_true", help="time the three existing calls only")
    ap.add_argument("--parent-json", help="the --existing-only result of the parent commit's library, to be merged in")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regression_posterior_timing.json"))
    args = ap.parse_args()
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    if args.existing_only:
        _lib._SIGNATURES.pop(NEW, None)
    torch.cuda.init()       # torch's HIP runtime opens the device before libflgp_hip.so does
    n, K, t, noise, sigma = 1_000_000, 200, 4.0, 0.1, 1e-3
    rng = np.random.default_rng(0)
    values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
    V = np.asfortranarray(rng.standard_normal((n, K)))
    rp = api.ResidentEigenPair.from_host(api.EigenPair(values, V))
    del V
    parent = json.load(open(args.parent_json)) if args.parent_json else None
    res = {"shape": dict(n=n, K=K, q=1, t=t, noise=noise, sigma=sigma), "reps": args.reps,
           "library": _lib.lib().flgp_version().decode(), "rows": []}
    for i, m in enumerate((1000, 10_000, 100_000)):
        idx0 = np.arange(m); idx1 = np.arange(m, n)
        Y = rng.standard_normal(m)
        pars = (t, noise)
        row = dict(m=m, m_new=n - m)

        def three():
            return (rp.predict_regression_cpp(Y, idx0, idx0, K, pars, sigma), rp.predict_regression_cpp(Y, idx0, idx1, K, pars, sigma),
                    rp.posterior_covariance_regression(idx0, idx1, K, pars, sigma))

        def new():
            return rp.regression_posterior(Y, idx0, idx1, K, pars, sigma)

        if not args.existing_only:
            row["regression_posterior"], out = timed(new, args.reps)
        row["three_existing_calls"], (tr, te, cv) = timed(three, args.reps)
        if not args.existing_only:
            row["regression_posterior"].update(
                max_abs_dtrain=float(np.abs(out["Y_pred"]["train"] - tr).max()), max_abs_dtest=float(np.abs(out["Y_pred"]["test"] - te).max()),
                max_abs_test=float(np.abs(te).max()), max_abs_dcov=float(np.abs(out["posterior"]["cov"] - cv).max()),
                min_cov_minus_c=float(out["posterior"]["cov"].min() - (noise + sigma)))
            row["regression_posterior_launches"] = prof_table(new)
        if parent:
            row["three_existing_calls_parent_library"] = parent["rows"][i]["three_existing_calls"]
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    rp.free()
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
