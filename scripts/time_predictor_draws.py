"""Timing of the joint posterior of served rows.  One process, HIP events around every call (and the wall
clock), a warm-up of every route first, the routes alternating, best of --reps with the slowest repetition beside it.

"kernel":  flgp_dev_predictor_cols against flgp_dev_predictor_pg_rows asked for f alone -- the kernel a wide P went through
           before -- on the same P (s = 5000 rows, random) and the same ELL rows (r = 10 sorted random anchors per row,
           random weights) of --new resident rows, at nc = 10, 64, 200, 1000 (and 320, 512, 768, to place the
           width from which flgp_dev_predictor_cols takes its tile kernel; the knob predictor_cols_tile_min is 1 here, so
           "cols" is the tile kernel at every width).  The bits are identical; the effective store bandwidth is n nc 8
           bytes over the event time.
"model":   BASELINE configs[2] -- Gaussian mixture, n = 1e6, d = 16, s = 5000 anchors, r = 10, K = 200, kernel "lae",
           gl "cluster-normalized", root TRUE -- as scripts/time_predictor.py fits it; a regression handle on the first
           m = 1000 rows, q = 1.  draws_create at S = 100 and 1000; flgp_dev_predictor_apply of those handles beside the
           source handle's mean-only apply; flgp_dev_predictor_features of --new rows; Predictor.covariance of 4096 x 4096
           rows (host entry: upload, features, GEMM, mirror, download).
"nystrom": the same three at s = 1e4 anchors, d = 64, K = 500, one bandwidth a2 = 1, a Gaussian cloud as
           scripts/time_nystrom_predictor.py draws it.
Writes one JSON object to --out (default profiles/predictor_draws_timing.json) and prints it.
Usage: python scripts/time_predictor_draws.py [--parts kernel,model,nystrom] [--new 100000] [--reps 7]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from flgp_amd import _lib, api, synth  # noqa: E402

MODELS = {"kernel": "lae", "gl": "cluster-normalized", "root": True}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, NOISE, SIGMA, SEED = 2.0, 0.1, 1e-3, 4242
TILE_MIN = 512                                               # the library's default of predictor_cols_tile_min


def timed(fn):
    """(result, HIP-event ms on the current stream, wall ms) of one library call, synchronised"""
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    w0 = time.perf_counter()
    e0.record(); out = fn(); e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1), (time.perf_counter() - w0) * 1e3


def race(routes, reps):
    """every route once to warm up, then reps rounds of all of them in turn: {name: best, slowest, wall of the best}"""
    for _, fn in routes:
        fn()
    best = {}
    for _ in range(reps):
        for name, fn in routes:
            _, ev, wall = timed(fn)
            slow = max(ev, best[name]["event_ms_slowest"]) if name in best else ev
            if name not in best or ev < best[name]["event_ms"]:
                best[name] = {"event_ms": ev, "wall_ms": wall}
            best[name]["event_ms_slowest"] = slow
    return best


def run_kernel(args):
    L = _lib.lib()
    n, s, r = args.new, 5000, 10
    rng = np.random.default_rng(7)
    idx = np.sort(rng.integers(0, s, size=(n, r)), axis=1).astype(np.int32)
    val = rng.uniform(0.0, 1.0, size=(n, r))
    d_idx, d_val = torch.from_numpy(idx).cuda(), torch.from_numpy(val).cuda()
    out = {"shape": {"n": n, "s": s, "r": r}, "widths": {}}
    L.flgp_set_tuning(b"predictor_cols_tile_min", 1)                            # the tile kernel at every width
    for nc in (10, 64, 200, 320, 512, 768, 1000):
        ldp = (nc + 15) // 16 * 16
        d_P = torch.from_numpy(rng.normal(size=(s, ldp))).cuda()
        a = torch.zeros((nc, n), device="cuda", dtype=torch.float64); b = torch.zeros((nc, n), device="cuda", dtype=torch.float64)
        st = torch.cuda.current_stream().cuda_stream

        def cols():
            _lib.check(L.flgp_dev_predictor_cols(st, d_idx.data_ptr(), d_val.data_ptr(), n, r, d_P.data_ptr(), ldp, s, 0, nc, a.data_ptr(), n))

        def pg_rows():
            _lib.check(L.flgp_dev_predictor_pg_rows(st, d_idx.data_ptr(), d_val.data_ptr(), n, r, d_P.data_ptr(), ldp, s, nc, b.data_ptr(), n,
                                                    None, 0, None, 0, None))

        res = race((("cols", cols), ("pg_rows_f", pg_rows)), args.reps)
        for k in res:
            res[k]["store_GB_per_s"] = 8e-6 * n * nc / res[k]["event_ms"]
        res["bits_equal"] = bool(torch.equal(a, b))
        res["pg_rows_over_cols"] = res["pg_rows_f"]["event_ms"] / res["cols"]["event_ms"]
        # the run-to-run spread of the two routes: the larger slowest-over-best gap
        res["spread"] = max(res[k]["event_ms_slowest"] / res[k]["event_ms"] for k in ("cols", "pg_rows_f"))
        out["widths"][str(nc)] = res
        del d_P, a, b
    L.flgp_set_tuning(b"predictor_cols_tile_min", TILE_MIN)
    out["tile_min_default"] = TILE_MIN
    return out


def joint(out, src, dXn, n_new, d, reps, X4k):
    """create, apply, features and covariance on the handle `src`"""
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    K = src.K
    dmean = torch.zeros((src.groups * src.q, n_new), device="cuda", dtype=torch.float64)
    dZ = torch.zeros((K, n_new), device="cuda", dtype=torch.float64)

    def mean_only():
        _lib.check(L.flgp_dev_predictor_apply(st, src._h, dXn.data_ptr(), n_new, n_new, dmean.data_ptr(), n_new, None, 0))

    def features():
        _lib.check(L.flgp_dev_predictor_features(st, src._h, 0, dXn.data_ptr(), n_new, n_new, dZ.data_ptr(), n_new))

    routes = [("source_mean_only_apply", mean_only), ("features", features)]
    handles, bufs = {}, {}
    for S in (100, 1000):
        src.draws(S, SEED).free()                                               # warm-up: the allocations of a create
        best, slow = None, 0.0
        for _ in range(reps):
            h, ev, wall = timed(lambda: src.draws(S, SEED))
            slow = max(slow, ev)
            if best is None or ev < best["event_ms"]:
                best = {"event_ms": ev, "wall_ms": wall}
            if S in handles:
                handles[S].free()
            handles[S] = h
        best["event_ms_slowest"] = slow
        best["P_draw_bytes"] = 8 * h.s * h.ldp
        out[f"draws_create_S{S}"] = best
        ncol = h.q
        bufs[S] = torch.zeros((ncol, n_new), device="cuda", dtype=torch.float64)

        def apply_draws(h=h, buf=bufs[S]):
            _lib.check(L.flgp_dev_predictor_apply(st, h._h, dXn.data_ptr(), n_new, n_new, buf.data_ptr(), n_new, None, 0))

        routes.append((f"draws_apply_S{S}", apply_draws))
    routes.append(("covariance_4096_host", lambda: src.covariance(X4k)))
    best = race(routes, reps)
    for S in (100, 1000):
        best[f"draws_apply_S{S}"]["store_GB_per_s"] = 8e-6 * n_new * handles[S].q / best[f"draws_apply_S{S}"]["event_ms"]
        best[f"draws_apply_S{S}"]["over_mean_only"] = best[f"draws_apply_S{S}"]["event_ms"] / best["source_mean_only_apply"]["event_ms"]
        handles[S].free()
    out.update(best)


def run_model(args):
    n, d, s, r, K, m, n_new = args.n, 16, 5000, 10, 200, args.m, args.new
    X = synth.gaussian_mixture(n, d)
    rows = np.sort(synth.random_anchor_rows(n, s))
    U0 = synth.anchors_from_rows(X, rows)
    sizes = np.bincount(api.KNN_cpp(X, U0, 1)["ind_knn"][:, 0], minlength=s).astype(float)
    U = np.asfortranarray(np.hstack([U0, sizes[:, None]]))
    model, pair = api.heat_kernel_spectrum_model(X, X[:0], s, r, K, models=MODELS, U=U)
    idx0 = np.arange(m, dtype=np.int32)
    Y = np.sin(2.0 * X[:m, :1])
    Xn = synth.gaussian_mixture(n_new, d, row_offset=n)
    dXn = torch.from_numpy(np.ascontiguousarray(Xn.T)).cuda()
    out = {"shape": {"n_fit": n, "d": d, "s": s, "r": r, "K": K, "m": m, "q": 1, "n_new": n_new}}
    src = api.Predictor.regression(model, pair, Y, idx0, K, (T, NOISE), SIGMA)
    joint(out, src, dXn, n_new, d, args.reps, np.asfortranarray(Xn[:4096]))
    src.free(); model.free(); pair.free()
    return out


def run_nystrom(args):
    d, s, K, m, n_new, a2 = 64, 10_000, 500, args.m, args.new, 1.0
    rng = np.random.default_rng(s + d)
    X = rng.normal(size=(max(m, s), d))
    U = X[rng.permutation(X.shape[0])[:s]] + 0.01 * rng.normal(size=(s, d))
    Xn = rng.normal(size=(n_new, d))
    grid = api.nystrom_spectrum_grid(U, (a2,), K, max_parallel=1)
    pair = grid.extend(0, X[:m], resident=True)
    idx0 = np.arange(m, dtype=np.int32)
    Y = np.sin(2.0 * X[:m, :1])
    dXn = torch.from_numpy(np.ascontiguousarray(Xn.T)).cuda()
    out = {"shape": {"d": d, "s": s, "K": K, "m": m, "q": 1, "n_new": n_new, "a2": a2}}
    src = api.Predictor.nystrom_regression(grid, 0, pair, Y, idx0, K, (T, NOISE), SIGMA)
    joint(out, src, dXn, n_new, d, args.reps, np.asfortranarray(Xn[:4096]))
    src.free(); pair.free(); grid.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kernel,model,nystrom")
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--new", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictor_draws_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_predictor_draws.py needs a GPU: a timing taken anywhere else says nothing")
    out = {}
    for part in args.parts.split(","):
        out[part] = {"kernel": run_kernel, "model": run_model, "nystrom": run_nystrom}[part](args)
        print(json.dumps({part: out[part]}, indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
