"""Timing of the logit posterior for a batch of problems in one call (flgp_eigenpair_logit_posterior_batch)
against the two routes a caller had before it: the one-vs-rest entry (flgp_eigenpair_logit_posterior_multiclass, f-12) at its
default four workers, and B calls of the binary entry (flgp_eigenpair_logit_posterior) with the host stacking.  A synthetic
resident pair with n = 1e6, K = 200; ten classes with balanced labels, ten values of t from 1 to 8, sigma11 = 0,
sigma22 = 1e-3, m = 1000 and 1e4, m_new = n - m.  The batch's problems are the one-vs-rest indicator columns: B = 1 is class
0, B = 10 the ten classes at their t (the multiclass entry's problems exactly), B = 40 every class at four of the ten t.
Prints one JSON object and writes it to profiles/logit_posterior_batch_timing.json.  Per m and B:

  * batch: the new entry, max_parallel = 0 (wall clock around the call: the uploads and the two m_new x B arrays coming down
    are in it);
  * binary: the B binary calls with their columns stacked into two m_new x B arrays;
  * multiclass (B = 10 only): the one-vs-rest entry at max_parallel = 4, with the spread (max - min) of its runs;
  * by HIP events on the entry's stream (flgp_prof), for the batch: the Newton iterations (logit_ws_batch_iter, count and
    summed device time) and the fused predictive pass (gpc_predict_rows_multi).

The blocks alternate in one process -- one run of every block per repetition, --reps repetitions after a warm-up of each --
and the best of each is reported beside its median and its spread.  After them, at B = 10, the batch and the multiclass
entry run --reps times each back to back (back_to_back_10), on all new rows and on 1000 of them: what a call costs when
nothing else ran before it, and the modes with their operands alone.

Usage: python scripts/time_logit_posterior_batch.py [--reps 5] [--out FILE]
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

BATCHES = (1, 10, 40)


def prof_sum(name):
    c = ctypes.c_int(); ms = ctypes.c_double(); w = ctypes.c_double()
    _lib.lib().flgp_prof_query(name.encode(), ctypes.addressof(c), ctypes.addressof(ms), ctypes.addressof(w))
    return c.value, ms.value


def alternate(blocks, reps):
    """One warm-up run of every block, then `reps` rounds of one run each in the given order; per block the best, the
    median and the spread (max - min) of its wall times in ms, and its last result."""
    out = {name: fn() for name, fn in blocks}
    times = {name: [] for name, _ in blocks}
    for _ in range(reps):
        for name, fn in blocks:
            t0 = time.perf_counter(); out[name] = fn(); times[name].append((time.perf_counter() - t0) * 1e3)
    stats = {name: dict(ms=min(t), median_ms=float(np.median(t)), spread_ms=max(t) - min(t), runs_ms=t) for name, t in times.items()}
    return stats, out


def device_ms(fn, reps, names):
    """best over reps profiled calls of the summed device time of each scope in `names`, and its count per call"""
    L = _lib.lib()
    best = {}
    for _ in range(reps):
        L.flgp_prof_reset(); L.flgp_prof_enable(2)
        fn()
        torch.cuda.synchronize(); L.flgp_prof_enable(0)
        for name in names:
            count, ms = prof_sum(name)
            if name not in best or ms < best[name]["ms"]:
                best[name] = dict(ms=ms, count=count)
    L.flgp_prof_reset()
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logit_posterior_batch_timing.json"))
    args = ap.parse_args()
    torch.cuda.init()       # torch's HIP runtime opens the device before libflgp_hip.so does
    n, K, J, s11, s22, tol, max_iter = 1_000_000, 200, 10, 0.0, 1e-3, 1e-5, 100
    ts10 = np.linspace(1.0, 8.0, J)
    rng = np.random.default_rng(0)
    values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
    V = np.asfortranarray(rng.standard_normal((n, K)))
    rp = api.ResidentEigenPair.from_host(api.EigenPair(values, V))
    del V
    res = {"shape": dict(n=n, K=K, J=J, ts=ts10.tolist(), sigma11=s11, sigma22=s22, tol=tol, max_iter=max_iter), "reps": args.reps,
           "rows": []}
    for m in (1000, 10_000):
        idx0 = np.arange(m); idx1 = np.arange(m, n)
        labels = rng.permutation(np.arange(m) % J).astype(np.float64)              # balanced labels
        ind = np.asfortranarray((labels[:, None] == np.arange(J)[None, :]).astype(np.float64))
        problems = {}
        for B in BATCHES:
            cols = (np.arange(B) % J).astype(np.int32)
            problems[B] = (cols, ts10[(cols + 3 * (np.arange(B) // J)) % J])

        def batch(B):
            cols, ts = problems[B]
            return rp.logit_posterior_batch(idx0, idx1, K, ts, ind, col=cols, sigma11=s11, sigma22=s22, tol=tol, max_iter=max_iter,
                                            return_iters=True)

        def binary(B):
            cols, ts = problems[B]
            mean = np.zeros((n - m, B), order="F"); cov = np.zeros((n - m, B), order="F"); its = []
            for b in range(B):
                post, it = rp.logit_posterior(idx0, idx1, K, ts[b], ind[:, cols[b]], s11, s22, tol, max_iter, return_iters=True)
                mean[:, b] = post["mean"]; cov[:, b] = post["cov"]; its.append(it)
            return {"mean": mean, "cov": cov}, np.array(its, dtype=np.int32)

        def multiclass():
            return rp.logit_posterior_multiclass(idx0, idx1, K, ts10, labels, s22, s11, tol, max_iter, 4, return_iters=True)

        blocks = []
        for B in BATCHES:
            blocks.append((f"batch_{B}", lambda B=B: batch(B)))
            if B == J:
                blocks.append(("multiclass_10_workers_4", multiclass))
            blocks.append((f"binary_{B}", lambda B=B: binary(B)))
        stats, out = alternate(blocks, args.reps)
        for B in BATCHES:       # the three routes return the same bytes
            (pb, ib), (ps, is_) = out[f"batch_{B}"], out[f"binary_{B}"]
            assert pb["mean"].tobytes() == ps["mean"].tobytes() and pb["cov"].tobytes() == ps["cov"].tobytes() and list(ib) == list(is_)
        pm, im = out["multiclass_10_workers_4"]
        assert pm["mean"].tobytes() == out["batch_10"][0]["mean"].tobytes() and list(im) == list(out["batch_10"][1])
        row = dict(m=m, m_new=n - m, wall=stats, iterations={str(B): [int(i) for i in out[f"batch_{B}"][1]] for B in BATCHES})
        row["device"] = {str(B): device_ms(lambda B=B: batch(B), args.reps, ("logit_ws_batch_iter", "gpc_predict_rows_multi"))
                         for B in BATCHES}
        # B = 10 once more without the alternation: each route --reps times back to back, on all new rows and on 1000 of them
        # (the modes and the operands alone: the pass is a few workgroups and the arrays coming down are small)
        few = idx1[:1000]
        row["back_to_back_10"] = {}
        for name, fn in (("batch", lambda: batch(J)), ("multiclass_workers_4", multiclass),
                         ("batch_1000_new_rows", lambda: rp.logit_posterior_batch(idx0, few, K, ts10, ind, sigma11=s11, sigma22=s22,
                                                                                  tol=tol, max_iter=max_iter)),
                         ("multiclass_1000_new_rows", lambda: rp.logit_posterior_multiclass(idx0, few, K, ts10, labels, s22, s11, tol,
                                                                                            max_iter, 4))):
            row["back_to_back_10"][name] = alternate([(name, fn)], args.reps)[0][name]
        mc = stats["multiclass_10_workers_4"]
        gain = mc["ms"] - stats["batch_10"]["ms"]
        row["batch_10_vs_multiclass"] = dict(gain_ms=gain, multiclass_spread_ms=mc["spread_ms"], faster=bool(gain > mc["spread_ms"]))
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    rp.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
