"""Timing of the fit_nystrom_* bandwidth loop (reference src/Fit.cpp:244-333) on device-resident data, two
routes in one process, HIP events around every call, one warm-up of each size first, the routes alternating:

  A  the per-bandwidth entry l + 1 times: flgp_dev_nystrom_eigenpair on the m training rows for every bandwidth, then on
     all n rows for the chosen one (it is timed twice: the difference is the run-to-run spread B is judged against);
  B  flgp_dev_nystrom_grid_create, _extend_all on the m training rows, _extend of the chosen bandwidth on all n rows --
     with max_parallel = 1 and with max_parallel = l.

Sizes: n = 1e6, d = 16, s = 5000, K = 200 and BASELINE configs[4] (n = 5e6, d = 64, s = 1e4, K = 500); m = 1e4, l = 10
bandwidths spaced as R/Fit.R:187-189 spaces its ten, between --a2-lo and --a2-hi: by default 0.5 .. 2, because on this
script's Gaussian clouds the ends of the reference's 0.1 .. 10 give spectra the eigensolver refuses (a2 = 10 at d = 16:
residuals above its tolerance after 80 outer iterations; the per-bandwidth entry refuses the same).  Prints one JSON object.

Usage: python scripts/time_nystrom_grid.py [--sizes small,c5] [--reps 1] [--chosen 5]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from flgp_amd import _lib  # noqa: E402

SIZES = {"small": dict(n=1_000_000, d=16, s=5000, K=200), "c5": dict(n=5_000_000, d=64, s=10_000, K=500)}


class Timed:
    """HIP events on the current stream around synchronous library calls"""

    def __init__(self):
        self.ms = {}

    def __call__(self, name, fn):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        self.ms[name] = self.ms.get(name, 0.0) + e0.elapsed_time(e1)


def run_size(cfg, m, a2s, chosen, reps):
    L = _lib.lib()
    n, d, s, K = cfg["n"], cfg["d"], cfg["s"], cfg["K"]
    l = a2s.size
    gen = torch.Generator(device="cuda").manual_seed(n + d)
    X = torch.randn((d, n), generator=gen, device="cuda", dtype=torch.float64)          # column-major n x d
    rows = torch.randperm(n, generator=gen, device="cuda")[:s]
    U = (X[:, rows] + 0.01 * torch.randn((d, s), generator=gen, device="cuda", dtype=torch.float64)).contiguous()
    Xm = X[:, :m].contiguous()
    val = torch.empty((l, K), device="cuda", dtype=torch.float64)
    vec_m = torch.empty((l, K, m), device="cuda", dtype=torch.float64)
    vec_n = torch.empty((K, n), device="cuda", dtype=torch.float64)
    st = torch.cuda.current_stream().cuda_stream

    def route_a():
        t = Timed()
        for i in range(l):
            t("train_rows", lambda: _lib.check(L.flgp_dev_nystrom_eigenpair(st, Xm.data_ptr(), m, m, d, U.data_ptr(), s, s, float(a2s[i]), K,
                                                                            val[i].data_ptr(), vec_m[i].data_ptr(), m)))
        t("all_rows", lambda: _lib.check(L.flgp_dev_nystrom_eigenpair(st, X.data_ptr(), n, n, d, U.data_ptr(), s, s, float(a2s[chosen]), K,
                                                                      val[chosen].data_ptr(), vec_n.data_ptr(), n)))
        t.ms["total"] = t.ms["train_rows"] + t.ms["all_rows"]
        return t.ms

    def route_b(max_parallel):
        t = Timed()
        h = ctypes.c_void_p(); workers = ctypes.c_int()
        t("create", lambda: _lib.check(L.flgp_dev_nystrom_grid_create(st, U.data_ptr(), s, s, d, a2s.ctypes.data, l, K, max_parallel,
                                                                      ctypes.byref(h))))
        try:
            t("extend_all", lambda: _lib.check(L.flgp_dev_nystrom_grid_extend_all(st, h, Xm.data_ptr(), m, m, val.data_ptr(),
                                                                                  vec_m.data_ptr(), m)))
            t("extend", lambda: _lib.check(L.flgp_dev_nystrom_grid_extend(st, h, chosen, X.data_ptr(), n, n, None, vec_n.data_ptr(), n)))
            _lib.check(L.flgp_nystrom_grid_dims(h, None, None, None, None, ctypes.byref(workers)))
        finally:
            L.flgp_nystrom_grid_free(h)
        t.ms["total"] = t.ms["create"] + t.ms["extend_all"] + t.ms["extend"]
        t.ms["workers"] = workers.value
        return t.ms

    route_b(1)                                            # warm-up: every kernel of both routes, the allocations
    best = {}
    for _ in range(reps):
        for name, fn in (("A_first", route_a), ("B_1", lambda: route_b(1)), ("A_second", route_a), ("B_l", lambda: route_b(l))):
            ms = fn()
            if name not in best or ms["total"] < best[name]["total"]:
                best[name] = ms
    spread = abs(best["A_first"]["total"] - best["A_second"]["total"])
    a_low = min(best["A_first"]["total"], best["A_second"]["total"])
    out = dict(shape=dict(cfg, m=m, l=l), **best)
    out["A_spread_ms"] = spread
    out["B_1_below_A_by_ms"] = a_low - best["B_1"]["total"]
    out["B_1_below_A_by_more_than_spread"] = bool(a_low - best["B_1"]["total"] > spread)
    out["B_1_stage_share"] = {k: best["B_1"][k] / best["B_1"]["total"] for k in ("create", "extend_all", "extend")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="small,c5")
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--m", type=int, default=10_000)
    ap.add_argument("--l", type=int, default=10)
    ap.add_argument("--a2-lo", type=float, default=0.5)
    ap.add_argument("--a2-hi", type=float, default=2.0)
    ap.add_argument("--chosen", type=int, default=5)
    args = ap.parse_args()
    torch.cuda.init()       # torch's HIP runtime opens the device before libflgp_hip.so does
    a2s = np.exp(np.linspace(np.log(args.a2_lo), np.log(args.a2_hi), args.l))
    res = {"a2s": a2s.tolist(), "chosen": args.chosen, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    for name in args.sizes.split(","):
        res[name] = run_size(SIZES[name], args.m, a2s, args.chosen, args.reps)
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
