"""Timing and deviation of the fitted spectrum model's extension against the only other way to get
eigenvector rows for points that were not in the fit: a refit on the stacked rows.  One process, HIP events around every
call (and the wall clock: the host entries include their uploads), a warm-up of every size first, the routes alternating,
best of --reps.

Fit: BASELINE configs[2] -- Gaussian mixture, n = 1e6, d = 16, s = 5000 anchors (seeded random rows, 1-NN cluster counts),
r = 10, K = 200, kernel "lae", gl "cluster-normalized", root TRUE.  New rows: a second draw of the same mixture (other rows
of the same seeded cloud).

  timing     for n_new in --new: `extend_resident` from host arrays (behind a head of the first m fit rows: the serving
             pair), the device-pointer entry on rows already in HBM, and `heat_kernel_spectrum_resident` on the n_fit +
             n_new stacked rows from host arrays.
  deviation  for --fractions of new rows: H = V e^{-t (1 - lambda)} V^T (sign-invariant) of `--hrows` new rows against
             `--hrows` fit rows, once from the extended pair and once from a refit on all rows with the same anchors and
             cluster sizes; max |dH| / max |H| at t = 1 and t = 4.  The fit here has --dev-n rows.  Beside it the same
             figure for a block of fit rows against fit rows (the fit's pair against the refit's): what the refit moves
             where nothing is extended.

Prints one JSON object.  Usage: python scripts/time_spectrum_extend.py [--n 1000000] [--new 1000,100000,1000000] [--reps 5]
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

from flgp_amd import _lib, api, synth  # noqa: E402

MODELS = {"kernel": "lae", "gl": "cluster-normalized", "root": True}


def timed(fn):
    """(result, HIP-event ms on the current stream, wall ms) of one synchronous library call"""
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    w0 = time.perf_counter()
    e0.record(); out = fn(); e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1), (time.perf_counter() - w0) * 1e3


def cloud(n, d, offset=0):
    return synth.gaussian_mixture(n, d, row_offset=offset)


def anchors(X, s):
    rows = np.sort(synth.random_anchor_rows(X.shape[0], s))
    U0 = synth.anchors_from_rows(X, rows)
    sizes = np.bincount(api.KNN_cpp(X, U0, 1)["ind_knn"][:, 0], minlength=s).astype(float)
    return np.asfortranarray(np.hstack([U0, sizes[:, None]]))


def better(best, name, ev, wall):
    """best (by the events) of the repetitions; the slowest repetition is kept beside it as the spread"""
    slow = max(ev, best[name]["event_ms_slowest"]) if name in best else ev
    if name not in best or ev < best[name]["event_ms"]:
        best[name] = {"event_ms": ev, "wall_ms": wall}
    best[name]["event_ms_slowest"] = slow


def timing(args):
    L = _lib.lib()
    n, d, s, r, K, m = args.n, args.d, args.s, args.r, args.K, args.m
    X = cloud(n, d)
    U = anchors(X, s)
    (model, pair), ev, wall = timed(lambda: api.heat_kernel_spectrum_model(X, X[:0], s, r, K, models=MODELS, U=U))
    out = {"fit": {"event_ms": ev, "wall_ms": wall, "n": n}}
    head_rows = np.arange(m)
    st = torch.cuda.current_stream().cuda_stream
    for n_new in args.new:
        Xn = cloud(n_new, d, offset=n)
        Xall = np.asfortranarray(np.vstack([X, Xn]))
        dXn = torch.from_numpy(np.ascontiguousarray(Xn.T)).cuda()                    # column-major n_new x d
        dvec = torch.empty((K, n_new), device="cuda", dtype=torch.float64)

        def ext_host():
            model.extend(Xn, resident=True, head=pair, head_rows=head_rows).free()

        def ext_dev():
            _lib.check(L.flgp_dev_spectrum_model_extend(st, model._h, dXn.data_ptr(), n_new, n_new, dvec.data_ptr(), n_new))

        def refit():                                                                 # the C entry itself: no host copy of the stack in the window
            h = ctypes.c_void_p()
            _lib.check(L.flgp_heat_kernel_spectrum_resident(Xall.ctypes.data, n + n_new, d, U.ctypes.data, s, d + 1, r, K, b"lae",
                                                            b"cluster-normalized", 1, 0.1, ctypes.byref(h)))
            L.flgp_eigenpair_free(h)
        routes = (("extend_resident_host", ext_host), ("extend_device", ext_dev), ("refit_stacked_host", refit))
        for _, fn in routes:                                                         # warm-up: kernels, allocations, pinned rings
            fn()
        best = {}
        for _ in range(args.reps):
            for name, fn in routes:
                _, ev, wall = timed(fn)
                better(best, name, ev, wall)
        best["refit_over_extend_host_wall"] = best["refit_stacked_host"]["wall_ms"] / best["extend_resident_host"]["wall_ms"]
        best["refit_over_extend_device_event"] = best["refit_stacked_host"]["event_ms"] / best["extend_device"]["event_ms"]
        out[f"n_new_{n_new}"] = best
        del dXn, dvec, Xall
        torch.cuda.empty_cache()
    model.free(); pair.free()
    return out


def deviation(args):
    n, d, s, r, K, h = args.dev_n, args.d, args.s, args.r, args.K, args.hrows
    X = cloud(n, d)
    U = anchors(X, s)
    model, pair = api.heat_kernel_spectrum_model(X, X[:0], s, r, K, models=MODELS, U=U)
    train = np.sort(synth.random_anchor_rows(n, h, seed=5))
    other = np.sort(synth.random_anchor_rows(n, h, seed=7))          # fit rows again: how far the refit moves H where nothing is extended
    out = {"n_fit": n, "hrows": h}
    for frac in args.fractions:
        n_new = int(round(frac * n))
        Xn = cloud(n_new, d, offset=n)
        new = np.sort(synth.random_anchor_rows(n_new, min(h, n_new), seed=6))
        ext = model.extend(Xn[new], resident=True, head=pair, head_rows=train)
        full = api.heat_kernel_spectrum_resident(X, Xn, s, r, K, models=MODELS, U=U)
        res = {"n_new": n_new}
        for t in (1.0, 4.0):
            He = ext.HK_from_spectrum_cpp(K, t, h + np.arange(new.size), np.arange(h))
            Hr = full.HK_from_spectrum_cpp(K, t, n + new, train)
            Hf, Hfr = pair.HK_from_spectrum_cpp(K, t, other, train), full.HK_from_spectrum_cpp(K, t, other, train)
            res[f"t{t:g}"] = {"max_abs_dH_over_max_abs_H": float(np.abs(He - Hr).max() / np.abs(Hr).max()), "max_abs_H": float(np.abs(Hr).max()),
                              "fit_rows_max_abs_dH_over_max_abs_H": float(np.abs(Hf - Hfr).max() / np.abs(Hfr).max())}
        ve, vr = ext.to_host().values, full.to_host().values
        res["max_abs_dvalues"] = float(np.abs(ve - vr).max())
        out[f"new_{frac:g}"] = res
        ext.free(); full.free()
    model.free(); pair.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--s", type=int, default=5000)
    ap.add_argument("--r", type=int, default=10)
    ap.add_argument("--K", type=int, default=200)
    ap.add_argument("--m", type=int, default=10_000)
    ap.add_argument("--new", type=lambda v: [int(float(x)) for x in v.split(",")], default=[1000, 100_000, 1_000_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dev-n", type=int, default=1_000_000)
    ap.add_argument("--fractions", type=lambda v: [float(x) for x in v.split(",")], default=[0.01, 0.1, 0.5])
    ap.add_argument("--hrows", type=int, default=512)
    ap.add_argument("--skip", default="", help="timing or deviation")
    args = ap.parse_args()
    torch.cuda.init()       # torch's HIP runtime opens the device before libflgp_hip.so does
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
           "shape": {"d": args.d, "s": args.s, "r": args.r, "K": args.K, "m": args.m, **MODELS}}
    if args.skip != "timing":
        res["timing"] = timing(args)
    if args.skip != "deviation":
        res["deviation"] = deviation(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
