"""Timing of the predictor's update.  One process, HIP events around every call (and the wall clock), a warm-up of
every route first, the routes alternating, best of --reps with the slowest repetition beside it.

"kernel":  flgp_dev_predictor_gram against the two-step route it fuses, on the same P (s = 5000 rows, random, K = 200, q = 1)
           and the same ELL rows (r = 10 sorted random anchors per row, random weights) of n_b = 1e3 and 1e5 resident rows:
           flgp_dev_predictor_cols into a stored n_b x (K + q) array (the kernel flgp_dev_predictor_features runs after the row
           chain, which both routes would share), then flgp_dev_gemm E^T E -- once with a split-K workspace (the faster way to
           run that product) and once without (the chain the Gram kernel reproduces per chunk).  The stored array's bytes are
           beside the times.
"model":   BASELINE configs[2] -- Gaussian mixture, n = 1e6, d = 16, s = 5000 anchors, r = 10, K = 200, kernel "lae", gl
           "cluster-normalized", root TRUE -- as scripts/time_predictor.py fits it; a regression handle on the first m = 1000
           rows, q = 1.  flgp_dev_predictor_update of n_b = 1e3 and 1e5 resident rows against the route the entries before it
           offer: SpectrumModel.extend of the n_b rows to a resident pair stacked under the m training rows, then
           Predictor.regression on the m + n_b rows (host entries: the times include the upload of the n_b x d rows).
Writes one JSON object to --out (default profiles/predictor_update_timing.json) and prints it.
Usage: python scripts/time_predictor_update.py [--parts kernel,model] [--reps 7]"""
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
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, NOISE, SIGMA = 2.0, 0.1, 1e-3
NBS = (1000, 100000)


def timed(fn):
    """(result, HIP-event ms on the current stream, wall ms) of one library call, synchronised"""
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    w0 = time.perf_counter()
    e0.record(); out = fn(); e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1), (time.perf_counter() - w0) * 1e3


def race(routes, reps, after=None):
    """every route once to warm up, then reps rounds of all of them in turn: {name: best, slowest, wall of the best}"""
    for name, fn in routes:
        r = fn()
        if after:
            after(name, r)
    best = {}
    for _ in range(reps):
        for name, fn in routes:
            r, ev, wall = timed(fn)
            if after:
                after(name, r)
            slow = max(ev, best[name]["event_ms_slowest"]) if name in best else ev
            if name not in best or ev < best[name]["event_ms"]:
                best[name] = {"event_ms": ev, "wall_ms": wall}
            best[name]["event_ms_slowest"] = slow
    return best


def ratio(res, slow, fast):
    """slow / fast of the best times, and the larger slowest-over-best gap of the two routes"""
    return {"ratio": res[slow]["event_ms"] / res[fast]["event_ms"],
            "spread": max(res[k]["event_ms_slowest"] / res[k]["event_ms"] for k in (slow, fast))}


def run_kernel(args):
    L = _lib.lib()
    s, r, K, q = 5000, 10, 200, 1
    W = K + q
    ldp = (W + 15) // 16 * 16
    rng = np.random.default_rng(7)
    d_P = torch.from_numpy(rng.normal(size=(s, ldp))).cuda()
    out = {"shape": {"s": s, "r": r, "K": K, "q": q}, "rows": {}}
    st = torch.cuda.current_stream().cuda_stream
    for n in NBS:
        idx = np.sort(rng.integers(0, s, size=(n, r)), axis=1).astype(np.int32)
        d_idx, d_val = torch.from_numpy(idx).cuda(), torch.from_numpy(rng.uniform(0.0, 1.0, size=(n, r))).cuda()
        d_w = torch.from_numpy(1.0 / rng.uniform(0.05, 0.5, size=n)).cuda()
        d_Y = torch.from_numpy(rng.normal(size=(q, n))).cuda()
        need = L.flgp_dev_predictor_gram_workspace(n, K, q)
        work = torch.zeros(need // 8, device="cuda", dtype=torch.float64)
        S = torch.zeros((W, W), device="cuda", dtype=torch.float64)
        E = torch.zeros((W, n), device="cuda", dtype=torch.float64)            # the array the fused kernel does not allocate
        C = torch.zeros((W, W), device="cuda", dtype=torch.float64)
        split = torch.zeros(64 * W * W, device="cuda", dtype=torch.float64)

        def gram():
            _lib.check(L.flgp_dev_predictor_gram(st, d_idx.data_ptr(), d_val.data_ptr(), n, r, d_P.data_ptr(), ldp, s, K, q, d_w.data_ptr(),
                                                 d_Y.data_ptr(), n, S.data_ptr(), W, work.data_ptr(), need))

        def two_step(ws, elems):
            _lib.check(L.flgp_dev_predictor_cols(st, d_idx.data_ptr(), d_val.data_ptr(), n, r, d_P.data_ptr(), ldp, s, 0, W, E.data_ptr(), n))
            _lib.check(L.flgp_dev_gemm(st, W, W, n, 1.0, E.data_ptr(), n, 1, E.data_ptr(), 1, n, 0.0, None, 0, 0, C.data_ptr(), 1, W, ws, elems))

        res = race((("gram", gram), ("cols_gemm_split", lambda: two_step(split.data_ptr(), split.numel())),
                    ("cols_gemm_chain", lambda: two_step(None, 0))), args.reps)
        res["split_over_gram"] = ratio(res, "cols_gemm_split", "gram")
        res["chain_over_gram"] = ratio(res, "cols_gemm_chain", "gram")
        res["stored_array_bytes"] = 8 * n * W
        res["gram_workspace_bytes"] = int(need)
        out["rows"][str(n)] = res
        del d_idx, d_val, d_w, d_Y, work, S, E, C, split
    return out


def run_model(args):
    n, d, s, r, K, m = args.n, 16, 5000, 10, 200, args.m
    L = _lib.lib()
    X = synth.gaussian_mixture(n, d)
    rows = np.sort(synth.random_anchor_rows(n, s))
    U0 = synth.anchors_from_rows(X, rows)
    sizes = np.bincount(api.KNN_cpp(X, U0, 1)["ind_knn"][:, 0], minlength=s).astype(float)
    U = np.asfortranarray(np.hstack([U0, sizes[:, None]]))
    model, pair = api.heat_kernel_spectrum_model(X, X[:0], s, r, K, models=MODELS, U=U)
    idx0 = np.arange(m, dtype=np.int32)
    Y = np.sin(2.0 * X[:m, :1])
    src = api.Predictor.regression(model, pair, Y, idx0, K, (T, NOISE), SIGMA)
    out = {"shape": {"n_fit": n, "d": d, "s": s, "r": r, "K": K, "m": m, "q": 1}, "rows": {}}
    st = torch.cuda.current_stream().cuda_stream
    for n_b in NBS:
        Xb = np.asfortranarray(synth.gaussian_mixture(n_b, d, row_offset=n))
        Yb = np.asfortranarray(np.sin(2.0 * Xb[:, :1]))
        dXb = torch.from_numpy(np.ascontiguousarray(Xb.T)).cuda(); dYb = torch.from_numpy(np.ascontiguousarray(Yb.T)).cuda()
        Yall = np.asfortranarray(np.vstack([Y, Yb]))
        all_rows = np.arange(m + n_b, dtype=np.int32)

        def update():
            o = ctypes.c_void_p()
            _lib.check(L.flgp_dev_predictor_update(st, src._h, dXb.data_ptr(), n_b, n_b, dYb.data_ptr(), n_b, None, 0, ctypes.byref(o)))
            return api.Predictor(o, model)

        def refit():
            stacked = model.extend(Xb, resident=True, head=pair, head_rows=idx0)
            h = api.Predictor.regression(model, stacked, Yall, all_rows, K, (T, NOISE), SIGMA)
            stacked.free()
            return h

        kept = {}

        def after(name, h):                                                     # each route's first handle: its P, for the record
            if name not in kept:
                kept[name] = h.to_host()["P"][:, :K + 1]
            h.free()

        res = race((("update", update), ("extend_and_create", refit)), args.reps, after)
        res["create_over_update"] = ratio(res, "extend_and_create", "update")
        res["max_abs_P_difference"] = float(np.abs(kept["update"] - kept["extend_and_create"]).max())
        res["max_abs_P"] = float(np.abs(kept["update"]).max())
        out["rows"][str(n_b)] = res
    src.free(); model.free(); pair.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kernel,model")
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictor_update_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_predictor_update.py needs a GPU: a timing taken anywhere else says nothing")
    out = {}
    for part in args.parts.split(","):
        out[part] = {"kernel": run_kernel, "model": run_model}[part](args)
        print(json.dumps({part: out[part]}, indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
