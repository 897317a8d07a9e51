"""Timing of the Polya-Gamma predictor against the serving route it replaces.  One process, HIP events around
every call (and the wall clock), a warm-up of every route first, the routes alternating, best of --reps with the slowest
repetition beside it.

"model":   BASELINE configs[2] -- Gaussian mixture, n = 1e6, d = 16, s = 5000 anchors, r = 10, K = 200, kernel "lae",
           gl "cluster-normalized", root TRUE -- as scripts/time_predictor.py fits it.
"nystrom": s = 1e4 anchors, d = 64, K = 500, one bandwidth a2 = 1, a Gaussian cloud as scripts/time_nystrom_predictor.py
           draws it.
Both: the first m = 1000 rows train ten one-vs-rest chains (classes: deciles of the first coordinate), N_sample = 100,
sigma = 1e-2; --new rows of another draw are resident on the device.

  route A   what serves a batch without the handle: the extension of the device rows (the n_new x K store), then
            flgp_eigenpair_pg_predict_batch on the pair of the training rows stacked on the new rows -- all N_sample sweeps
            again.  The two calls are timed separately; A is their sum.
  route B   flgp_dev_predictor_pg_apply on the same device rows: pi, y and label from the handle.
  create    Predictor.pg / .nystrom_pg once: the sweeps and the fold.

break_even_batches: the smallest number of batches from which create + k B <= k A.  Labels of A and B are compared on the
timed rows.  Writes one JSON object to --out (default profiles/predictor_pg_timing.json) and prints it.
Usage: python scripts/time_predictor_pg.py [--parts model,nystrom] [--new 100000] [--reps 7]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from flgp_amd import _lib, api, synth  # noqa: E402

MODELS = {"kernel": "lae", "gl": "cluster-normalized", "root": True}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA, SEED = 1e-2, 4242


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


def classes_of(x, J):
    return np.minimum((np.argsort(np.argsort(x)) * J) // x.size, J - 1).astype(np.float64)


def race(out, extend, both, pred, make, labels, ts, K, m, n_new, dXn, reps, n_sample):
    """routes A and B on the same rows; `make` builds the handle again for the create time"""
    L = _lib.lib()
    J = ts.size
    st = torch.cuda.current_stream().cuda_stream
    i0, i1 = np.arange(m, dtype=np.int32), (m + np.arange(n_new)).astype(np.int32)
    dpi = torch.empty((J, n_new), device="cuda", dtype=torch.float64); dy = torch.empty((J, n_new), device="cuda", dtype=torch.float64)
    dlab = torch.empty(n_new, device="cuda", dtype=torch.float64)

    def a_chains():
        return both.predict_logit_mult_gp_batch(i0, i1, K, ts, labels, SIGMA, N_sample=n_sample, seed=SEED, output_probs=True)

    def b_apply():
        _lib.check(L.flgp_dev_predictor_pg_apply(st, pred._h, dXn.data_ptr(), n_new, n_new, None, 0, dpi.data_ptr(), n_new,
                                                 dy.data_ptr(), n_new, dlab.data_ptr()))

    routes = (("A_extend_device", extend), ("A_pg_predict_batch", a_chains), ("B_predictor_pg_apply_device", b_apply))
    for _, fn in routes:
        fn()
    best = {}
    for _ in range(reps):
        for name, fn in routes:
            _, ev, wall = timed(fn)
            better(best, name, ev, wall)
    again, ev, wall = timed(make)
    again.free()
    out["create"] = {"event_ms": ev, "wall_ms": wall, "P_bytes": 8 * pred.s * pred.ldp}
    out.update(best)
    a_ev = best["A_extend_device"]["event_ms"] + best["A_pg_predict_batch"]["event_ms"]
    b_ev = best["B_predictor_pg_apply_device"]["event_ms"]
    out["A_total"] = {"event_ms": a_ev, "wall_ms": best["A_extend_device"]["wall_ms"] + best["A_pg_predict_batch"]["wall_ms"]}
    out["A_over_B_event"] = a_ev / b_ev
    out["A_over_B_wall"] = out["A_total"]["wall_ms"] / best["B_predictor_pg_apply_device"]["wall_ms"]
    out["us_per_row"] = {"A": 1e3 * a_ev / n_new, "B": 1e3 * b_ev / n_new}
    out["break_even_batches"] = int(math.ceil(ev / (a_ev - b_ev))) if a_ev > b_ev else None
    lab, probs = a_chains()
    b_apply(); torch.cuda.synchronize()
    out["labels_equal_fraction"] = float((dlab.cpu().numpy() == lab).mean())
    out["max_abs_dpi"] = float(np.abs(dpi.cpu().numpy().T - probs).max())


def run_model(args):
    L = _lib.lib()
    n, d, s, r, K, m, n_new, J = args.n, 16, 5000, 10, 200, args.m, args.new, args.classes
    X = synth.gaussian_mixture(n, d)
    rows = np.sort(synth.random_anchor_rows(n, s))
    U0 = synth.anchors_from_rows(X, rows)
    sizes = np.bincount(api.KNN_cpp(X, U0, 1)["ind_knn"][:, 0], minlength=s).astype(float)
    U = np.asfortranarray(np.hstack([U0, sizes[:, None]]))
    model, pair = api.heat_kernel_spectrum_model(X, X[:0], s, r, K, models=MODELS, U=U)
    idx0 = np.arange(m, dtype=np.int32)
    labels = classes_of(X[:m, 0], J)
    ts = np.full(J, 2.0)
    Xn = synth.gaussian_mixture(n_new, d, row_offset=n)
    dXn = torch.from_numpy(np.ascontiguousarray(Xn.T)).cuda()
    dvec = torch.empty((K, n_new), device="cuda", dtype=torch.float64)
    st = torch.cuda.current_stream().cuda_stream
    both = model.extend(Xn, resident=True, head=pair, head_rows=idx0)
    out = {"shape": {"n_fit": n, "d": d, "s": s, "r": r, "K": K, "m": m, "chains": J, "N_sample": args.n_sample, "n_new": n_new,
                     "sigma": SIGMA}}

    def make():
        return api.Predictor.pg_for_classes(model, pair, idx0, K, ts, labels, SIGMA, N_sample=args.n_sample, seed=SEED)

    def extend():
        _lib.check(L.flgp_dev_spectrum_model_extend(st, model._h, dXn.data_ptr(), n_new, n_new, dvec.data_ptr(), n_new))

    pred = make()
    race(out, extend, both, pred, make, labels, ts, K, m, n_new, dXn, args.reps, args.n_sample)
    pred.free(); both.free(); model.free(); pair.free()
    return out


def run_nystrom(args):
    L = _lib.lib()
    d, s, K, m, n_new, J, a2 = 64, 10_000, 500, args.m, args.new, args.classes, 1.0
    rng = np.random.default_rng(s + d)
    X = rng.normal(size=(max(m, s), d))
    U = X[rng.permutation(X.shape[0])[:s]] + 0.01 * rng.normal(size=(s, d))
    Xn = rng.normal(size=(n_new, d))
    grid = api.nystrom_spectrum_grid(U, (a2,), K, max_parallel=1)
    pair = grid.extend(0, X[:m], resident=True)
    both = grid.extend(0, np.vstack([X[:m], Xn]), resident=True)
    idx0 = np.arange(m, dtype=np.int32)
    labels = classes_of(X[:m, 0], J)
    ts = np.full(J, 2.0)
    dXn = torch.from_numpy(np.ascontiguousarray(Xn.T)).cuda()
    dvec = torch.empty((K, n_new), device="cuda", dtype=torch.float64)
    st = torch.cuda.current_stream().cuda_stream
    out = {"shape": {"d": d, "s": s, "K": K, "m": m, "chains": J, "N_sample": args.n_sample, "n_new": n_new, "a2": a2, "sigma": SIGMA}}

    def make():
        return api.Predictor.nystrom_pg_for_classes(grid, 0, pair, idx0, K, ts, labels, SIGMA, N_sample=args.n_sample, seed=SEED)

    def extend():
        _lib.check(L.flgp_dev_nystrom_grid_extend(st, grid._h, 0, dXn.data_ptr(), n_new, n_new, None, dvec.data_ptr(), n_new))

    pred = make()
    race(out, extend, both, pred, make, labels, ts, K, m, n_new, dXn, args.reps, args.n_sample)
    pred.free(); both.free(); pair.free(); grid.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="model,nystrom")
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--new", type=int, default=100000)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--n-sample", dest="n_sample", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictor_pg_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_predictor_pg.py needs a GPU: a timing taken anywhere else says nothing")
    out = {}
    for part in args.parts.split(","):
        out[part] = {"model": run_model, "nystrom": run_nystrom}[part](args)
        print(json.dumps({part: out[part]}, indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
