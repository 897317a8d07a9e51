"""Timing of the batched regression training objective (flgp_regression_batch_*) against the route it
replaces, on ten synthetic resident pairs with n = 1e6, K = 200 and q = 1:

  * route A: B calls of the unchanged single entry flgp_eigenpair_regression_objective, one after another;
  * route B: one eval on a context made once (max_parallel = 0: one chunk where the memory allows);
  * m = 1000 and 1e4, noise "same" and "different", value plus gradient;
  * B = 1, 10 (the ten pairs at one x each) and 40 (the ten pairs cycled, four x each).

Same process, the two routes alternating, best of --reps after one warm-up of each.  Per row: both times, route A's
run-to-run spread (max - min over its reps), the create time of the context (reported apart: it is paid once per grid) and
whether every value and gradient of the batch equals the single calls' bit for bit.  Writes one JSON object to --out.

--trace: no timing; at m = --trace-m, noise "same", one warm-up and then ONE eval of a B = 1 context followed by ONE eval of
a B = 10 context, for a kernel trace of the run (rocprofv3 --kernel-trace --stats -- python scripts/...).
--count DIR: no GPU work; reads the kernel trace under DIR and prints the launches of the last two evaluations (from
rgb_weights_kernel to rgb_assemble_kernel, both included), to be merged into the JSON with --launches.

Usage: python scripts/time_regression_objective_batch.py [--reps 5] [--out profiles/regression_objective_batch_timing.json]
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def count_launches(folder):
    """kernels per evaluation from a rocprofv3 kernel trace: every run of kernels from rgb_weights_kernel to
    rgb_assemble_kernel, in start order"""
    rows = []
    for path in glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    evals, cur = [], None
    for _, name in rows:
        if "rgb_weights_kernel" in name:
            cur = {}
        if cur is not None:
            short = name.split("(")[0].split("::")[-1]
            cur[short] = cur.get(short, 0) + 1
            if "rgb_assemble_kernel" in name:
                evals.append(cur)
                cur = None
    return evals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regression_objective_batch_timing.json"))
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-m", type=int, default=1000)
    ap.add_argument("--count", default=None)
    ap.add_argument("--launches", default=None, help="a JSON file written by --count, merged into --out")
    args = ap.parse_args()
    if args.count:
        evals = count_launches(args.count)
        out = {"evaluations_traced": len(evals)}
        for B, e in zip((1, 10), evals[-2:]):
            out["B=%d" % B] = {"launches": sum(e.values()), "kernels": e}
        print(json.dumps(out, indent=1))
        return
    if args.launches:
        with open(args.out) as fh:
            res = json.load(fh)
        with open(args.launches) as fh:
            res["launches_per_eval_m1000_same"] = json.load(fh)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
        return

    import torch
    from flgp_amd import api
    torch.cuda.init()       # torch's HIP runtime opens the device before libflgp_hip.so does
    n, K, sigma = args.n, 200, 1e-5
    rng = np.random.default_rng(0)
    base = np.asfortranarray(rng.standard_normal((n, K)))
    pairs = []
    for p in range(10):      # ten distinct pairs: the base rows rolled, values of their own
        values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
        pairs.append(api.ResidentEigenPair.from_host(api.EigenPair(values, np.asfortranarray(np.roll(base, 1000 * p, axis=0)))))
    del base

    def problems(B, m, noise):
        rps = [pairs[b % 10] for b in range(B)]
        X = np.array([np.r_[rng.uniform(1.0, 6.0), rng.uniform(0.05, 0.4, 1 if noise == "same" else m)] for _ in range(B)])
        return rps, X

    def routes(rps, X, m, noise, idx, Y):
        def single():
            out = [rp.regression_objective(x, K, idx, Y, sigma=sigma, noise=noise) for rp, x in zip(rps, X)]
            return np.array([o[0] for o in out]), np.array([o[1] for o in out])
        t0 = time.perf_counter()
        ctx = api.RegressionObjectiveBatch(rps, K, idx, Y, sigma=sigma, noise=noise)
        create = time.perf_counter() - t0
        return single, (lambda: ctx(X)), ctx, create

    if args.trace:
        m = args.trace_m
        idx = rng.choice(n, m, replace=False)
        Y = rng.standard_normal((m, 1))
        for B in (1, 10):
            rps, X = problems(B, m, "same")
            _, batch, ctx, _ = routes(rps, X, m, "same", idx, Y)
            if B == 1:
                batch()      # the warm-up: module load and the GEMM's first launch
            batch()
            ctx.free()
        for rp in pairs:
            rp.free()
        print(json.dumps({"trace_m": m, "evals": ["warm-up B=1", "B=1", "B=10"]}))
        return

    res = {"shape": dict(n=n, K=K, q=1, pairs=10), "sigma": sigma, "reps": args.reps, "max_parallel": 0, "rows": []}
    for m in (1000, 10_000):
        idx = rng.choice(n, m, replace=False)
        Y = rng.standard_normal((m, 1))
        for noise in ("same", "different"):
            for B in (1, 10, 40):
                rps, X = problems(B, m, noise)
                single, batch, ctx, create = routes(rps, X, m, noise, idx, Y)
                ref = single(); got = batch()                                   # the warm-up of both routes
                ta, tb = [], []
                for _ in range(args.reps):                                      # alternating
                    t0 = time.perf_counter(); ref = single(); ta.append(time.perf_counter() - t0)
                    t0 = time.perf_counter(); got = batch(); tb.append(time.perf_counter() - t0)
                a, b = min(ta) * 1e3, min(tb) * 1e3
                row = {"m": m, "noise": noise, "B": B, "chunk": ctx.chunk, "single_calls_ms": a,
                       "single_calls_median_ms": float(np.median(ta)) * 1e3, "single_calls_spread_ms": (max(ta) - min(ta)) * 1e3,
                       "batch_ms": b, "batch_median_ms": float(np.median(tb)) * 1e3, "batch_spread_ms": (max(tb) - min(tb)) * 1e3,
                       "speedup": a / b, "gain_exceeds_spread": bool(a - b > max(ta) - min(ta)),
                       "loss_within_spread": bool(b - a <= max(ta) - min(ta)), "create_ms": create * 1e3,
                       "bits_equal": bool(ref[0].tobytes() == got[0].tobytes() and ref[1].tobytes() == got[1].tobytes())}
                ctx.free()
                res["rows"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
    for rp in pairs:
        rp.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
