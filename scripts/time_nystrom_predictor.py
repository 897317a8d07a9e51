"""Timing of the Nystrom predictor against the serving route it replaces.  One process, HIP events around
every call (and the wall clock), a warm-up of every route first, the routes alternating, best of --reps with the slowest
repetition beside it.

Shapes: "c5" -- s = 1e4 anchors, d = 64, K = 500 (BASELINE configs[4]) -- and "small" -- s = 5000, d = 16, K = 200; Gaussian
clouds as scripts/time_nystrom_grid.py draws them, one bandwidth a2 = 1, m = 1e4 training rows (q = 1), 1e5 new rows of
another draw resident on the device.

  route A   flgp_dev_nystrom_grid_extend on the device rows (Z block by block, the n_new x K store), then
            regression_posterior on the pair of the training rows stacked on the new rows.  The two calls are timed
            separately; A is their sum.
  route B   flgp_dev_predictor_apply on the same device rows, the mean alone.
  route C   the same, mean and variance.
  route D   Predictor.nystrom_regression, once.
  route E   a ten-group logit handle (one-vs-rest classes), its create once and its apply, the mean alone.

Per route the algorithmic operations and bytes per row are computed from the shape (see `per_row`).  A and C are compared on
the timed rows (max |d| relative to max |value|).  Writes one JSON object to --out and prints it.
Usage: python scripts/time_nystrom_predictor.py [--sizes c5,small] [--new 100000] [--reps 7]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from flgp_amd import _lib, api  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"c5": dict(d=64, s=10_000, K=500), "small": dict(d=16, s=5000, K=200)}


def timed(fn):
    """(result, HIP-event ms on the current stream, wall ms) of one synchronous library call"""
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    w0 = time.perf_counter()
    e0.record(); out = fn(); e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1), (time.perf_counter() - w0) * 1e3


def better(best, name, ev, wall):
    slow = max(ev, best[name]["event_ms_slowest"]) if name in best else ev
    if name not in best or ev < best[name]["event_ms"]:
        best[name] = {"event_ms": ev, "wall_ms": wall}
    best[name]["event_ms_slowest"] = slow


def per_row(d, s, K, q, groups, gemm_dots):
    """algorithmic floating-point operations and bytes of device memory traffic per new row (8-byte doubles; the anchors,
    P and the operand are shared by the rows of a block and not counted).  sim: 2 dpad for the dot product, 4 for the
    distance and the exponent, exp counted as one, 4 for the two row sums.  Where the dot products come from the GEMM
    they are stored and read once (16 s bytes); a stored Z is 8 s written and 8 s read per GEMM that consumes it."""
    dpad = next(p for p in (4, 8, 16, 32, 64, (d + 7) // 8 * 8) if d <= p)
    sim = s * (2 * dpad + 9)
    chunks = -(-s // 64)
    dots = 16 * s if gemm_dots else 0
    w = K + q
    return {
        "A_extend": {"flop": sim + 2 * s * K + K, "bytes": 8 * d + dots + 16 * s + 8 * K + 32 * chunks},
        "A_posterior": {"flop": 2 * K * w + 2 * K, "bytes": 8 * K + 8 * (q + 1)},
        "B_mean": {"flop": sim + 2 * s * groups * q, "bytes": 8 * d + dots + 16 * chunks * (2 + 8 * -(-groups * q // 8)) + 8 * groups * q},
        "C_mean_var": {"flop": sim + 2 * s * groups * q + 2 * s * groups * w + 3 * groups * K,
                       "bytes": 8 * d + max(dots, 8 * s) + 8 * s + 16 * groups * w + 16 * chunks * (2 + 8 * -(-groups * q // 8))
                       + 8 * groups * (q + 1)},
    }


def run_size(name, cfg, m, n_new, reps, J):
    L = _lib.lib()
    d, s, K = cfg["d"], cfg["s"], cfg["K"]
    t, noise, sigma, a2 = 2.0, 0.1, 1e-3, 1.0
    rng = np.random.default_rng(s + d)
    X = rng.normal(size=(m, d))
    U = X[rng.permutation(m)[:s]] + 0.01 * rng.normal(size=(s, d))
    Xn = rng.normal(size=(n_new, d))
    Y = np.asfortranarray(np.sin(2.0 * X[:, :1]) + 0.1 * rng.normal(size=(m, 1)))
    idx0 = np.arange(m, dtype=np.int32)
    grid, ev, wall = timed(lambda: api.nystrom_spectrum_grid(U, (a2,), K, max_parallel=1))
    out = {"shape": {"d": d, "s": s, "K": K, "m": m, "q": 1, "n_new": n_new, "a2": a2, "t": t, "noise": noise, "sigma": sigma},
           "grid_create": {"event_ms": ev, "wall_ms": wall}}
    gemm_dots = d > 32
    out["per_row"] = per_row(d, s, K, 1, 1, gemm_dots)
    out["per_row"]["E_mean_ten_groups"] = per_row(d, s, K, 1, J, gemm_dots)["B_mean"]
    pair = grid.extend(0, X, resident=True)
    both = grid.extend(0, np.vstack([X, Xn]), resident=True)                         # the pair route A's posterior reads
    i1 = (m + np.arange(n_new)).astype(np.int32)
    dXn = torch.from_numpy(np.ascontiguousarray(Xn.T)).cuda()                        # column-major n_new x d
    dvec = torch.empty((K, n_new), device="cuda", dtype=torch.float64)
    dmean = torch.empty((1, n_new), device="cuda", dtype=torch.float64); dvar = torch.empty((1, n_new), device="cuda", dtype=torch.float64)
    st = torch.cuda.current_stream().cuda_stream

    pred, ev, wall = timed(lambda: api.Predictor.nystrom_regression(grid, 0, pair, Y, idx0, K, (t, noise), sigma))
    out["D_create_regression"] = {"event_ms": ev, "wall_ms": wall, "P_bytes": 8 * pred.s * pred.ldp}

    def a_extend():
        _lib.check(L.flgp_dev_nystrom_grid_extend(st, grid._h, 0, dXn.data_ptr(), n_new, n_new, None, dvec.data_ptr(), n_new))

    def a_posterior():
        return both.regression_posterior(Y, idx0, i1, K, (t, noise), sigma, train=False)

    def b_mean():
        _lib.check(L.flgp_dev_predictor_apply(st, pred._h, dXn.data_ptr(), n_new, n_new, dmean.data_ptr(), n_new, None, n_new))

    def c_both():
        _lib.check(L.flgp_dev_predictor_apply(st, pred._h, dXn.data_ptr(), n_new, n_new, dmean.data_ptr(), n_new, dvar.data_ptr(), n_new))

    routes = (("A_extend_device", a_extend), ("A_regression_posterior", a_posterior), ("B_apply_mean", b_mean),
              ("C_apply_mean_var", c_both))
    for _, fn in routes:
        fn()
    best = {}
    for _ in range(reps):
        for rname, fn in routes:
            _, ev, wall = timed(fn)
            better(best, rname, ev, wall)
    out.update(best)
    a_ev = best["A_extend_device"]["event_ms"] + best["A_regression_posterior"]["event_ms"]
    out["A_total"] = {"event_ms": a_ev, "wall_ms": best["A_extend_device"]["wall_ms"] + best["A_regression_posterior"]["wall_ms"]}
    out["A_over_B_event"] = a_ev / best["B_apply_mean"]["event_ms"]
    out["A_over_C_event"] = a_ev / best["C_apply_mean_var"]["event_ms"]
    out["us_per_row"] = {"A": 1e3 * a_ev / n_new, "B": 1e3 * best["B_apply_mean"]["event_ms"] / n_new,
                         "C": 1e3 * best["C_apply_mean_var"]["event_ms"] / n_new}
    ref = a_posterior()["posterior"]
    c_both(); torch.cuda.synchronize()
    out["A_vs_C_max_abs_dmean_over_max_abs_mean"] = float(np.abs(dmean.cpu().numpy()[0] - ref["mean"][:, 0]).max() / np.abs(ref["mean"]).max())
    out["A_vs_C_max_abs_dvar_over_max_abs_var"] = float(np.abs(dvar.cpu().numpy()[0] - ref["cov"]).max() / np.abs(ref["cov"]).max())
    pred.free(); both.free()
    del dvec

    # ten one-vs-rest classes: groups = 10, the mean alone (ten columns: two passes of the mean kernel)
    labels = np.minimum((np.argsort(np.argsort(X[:, 0])) * J) // m, J - 1)
    Yc = np.asfortranarray((labels[:, None] == np.arange(J)[None, :]).astype(np.float64))
    predc, ev, wall = timed(lambda: api.Predictor.nystrom_logit(grid, 0, pair, idx0, K, np.full(J, t), Yc))
    out["E_create_logit"] = {"event_ms": ev, "wall_ms": wall, "groups": J, "P_bytes": 8 * predc.s * predc.ldp,
                             "iters": [int(i) for i in predc.iters]}
    cmean = torch.empty((J, n_new), device="cuda", dtype=torch.float64)

    def e_mean():
        _lib.check(L.flgp_dev_predictor_apply(st, predc._h, dXn.data_ptr(), n_new, n_new, cmean.data_ptr(), n_new, None, n_new))
    e_mean()
    beste = {}
    for _ in range(reps):
        _, ev, wall = timed(e_mean)
        better(beste, "E_apply_mean_ten_groups", ev, wall)
    out.update(beste)
    predc.free(); pair.free(); grid.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="c5,small")
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--new", type=int, default=100000)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nystrom_predictor_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_nystrom_predictor.py needs a GPU: a timing taken anywhere else says nothing")
    out = {}
    for name in args.sizes.split(","):
        out[name] = run_size(name, SIZES[name], args.m, args.new, args.reps, args.classes)
        text = json.dumps(out, indent=1)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:                       # (after every size: a later size that fails loses nothing)
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
