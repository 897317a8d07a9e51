"""Timing of the greedy variance design.  One process, HIP events around every call (and the wall clock), a
warm-up of every route first, the routes alternating, best of --reps with the slowest repetition beside it.

The model is BASELINE configs[2] -- Gaussian mixture, n = 1e6, d = 16, s = 5000 anchors, r = 10, K = 200, kernel "lae", gl
"cluster-normalized", root TRUE -- as scripts/time_predictor_update.py fits it; a regression handle on the first m = 1000 rows,
q = 1.  Pools of 1e5 and 1e6 rows resident on the device, B in {10, 100, 1000}:

"design"    flgp_dev_predictor_design: the row chain of the pool, then the loop;
"loop"      flgp_dev_predictor_design_rows alone, on the handle's P and random ELL rows of the pool's shape (r sorted random
            anchors per row, random weights); per step = (time at B = 1000 - time at B = 100) / 900; "loop_rows_in_place" is the
            same with the knob predictor_design_pack at 0: the row-major arrays read with lane = row, no transposed copy;
"one_pick"  the route this entry replaces, one pick of it: flgp_dev_predictor_update on one row, flgp_dev_predictor_apply
            (variance) on the pool, an argmax on the device; run as a chain of 10 picks, reported per pick (B picks cost B times
            that: the update does not grow with the labels seen);
"features"  flgp_dev_predictor_features of the pool into a stored n x K array (what a pivoted Cholesky on the host would start
            from), with that array's bytes.
Writes one JSON object to --out (default profiles/predictor_design_timing.json) and prints it.
Usage: python scripts/time_predictor_design.py [--reps 7] [--pools 100000,1000000]"""
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
BS = (10, 100, 1000)


def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    w0 = time.perf_counter()
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - w0) * 1e3


def race(routes, reps):
    """every route once to warm up, then reps rounds of all of them in turn: {name: best, slowest, wall of the best}"""
    for _, fn in routes:
        fn()
    best = {}
    for _ in range(reps):
        for name, fn in routes:
            ev, wall = timed(fn)
            slow = max(ev, best[name]["event_ms_slowest"]) if name in best else ev
            if name not in best or ev < best[name]["event_ms"]:
                best[name] = {"event_ms": ev, "wall_ms": wall}
            best[name]["event_ms_slowest"] = slow
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pools", default="100000,1000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictor_design_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_predictor_design.py needs a GPU: a timing taken anywhere else says nothing")
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
    ldp = src.ldp
    d_P = torch.from_numpy(src.to_host()["P"]).cuda()
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(11)
    out = {"shape": {"n_fit": n, "d": d, "s": s, "r": r, "K": K, "m": m, "q": 1, "noise": NOISE, "sigma": SIGMA}, "pools": {}}
    for pool in (int(v) for v in args.pools.split(",")):
        Xp = np.asfortranarray(synth.gaussian_mixture(pool, d, row_offset=n))
        dX = torch.from_numpy(np.ascontiguousarray(Xp.T)).cuda()
        idx = np.sort(rng.integers(0, s, size=(pool, r)), axis=1).astype(np.int32)
        d_idx, d_val = torch.from_numpy(idx).cuda(), torch.from_numpy(rng.uniform(0.0, 1.0, size=(pool, r)) / r).cuda()
        picks = torch.zeros(max(BS), dtype=torch.int32, device="cuda")
        gain = torch.zeros(max(BS), dtype=torch.float64, device="cuda")
        score = torch.zeros(pool, dtype=torch.float64, device="cuda")
        var = torch.zeros(pool, dtype=torch.float64, device="cuda")
        y1 = torch.zeros(1, dtype=torch.float64, device="cuda")
        x1 = torch.zeros(d, dtype=torch.float64, device="cuda")
        need = {B: L.flgp_dev_predictor_design_workspace(pool, r, s, K, B) for B in BS}
        work = torch.zeros(max(need.values()) // 8, dtype=torch.float64, device="cuda")

        def design(B):
            _lib.check(L.flgp_dev_predictor_design(st, src._h, dX.data_ptr(), pool, pool, B, None, picks.data_ptr(), gain.data_ptr(),
                                                   score.data_ptr()))

        def loop(B):
            _lib.check(L.flgp_dev_predictor_design_rows(st, d_idx.data_ptr(), d_val.data_ptr(), pool, r, d_P.data_ptr(), ldp, s, K,
                                                        NOISE + SIGMA, B, picks.data_ptr(), gain.data_ptr(), score.data_ptr(),
                                                        work.data_ptr(), need[B]))

        def ten_picks():
            h = src
            for _ in range(10):
                _lib.check(L.flgp_dev_predictor_apply(st, h._h, dX.data_ptr(), pool, pool, None, 0, var.data_ptr(), pool))
                j = torch.argmax(var)
                x1.copy_(dX[:, j])
                o = ctypes.c_void_p()
                _lib.check(L.flgp_dev_predictor_update(st, h._h, x1.data_ptr(), 1, 1, y1.data_ptr(), 1, None, 0, ctypes.byref(o)))
                if h is not src:
                    h.free()
                h = api.Predictor(o, model)
            h.free()

        Z = torch.zeros((K, pool), dtype=torch.float64, device="cuda")

        def features():
            _lib.check(L.flgp_dev_predictor_features(st, src._h, 0, dX.data_ptr(), pool, pool, Z.data_ptr(), pool))

        def loop_in_place(B):
            L.flgp_set_tuning(b"predictor_design_pack", 0)
            try:
                loop(B)
            finally:
                L.flgp_set_tuning(b"predictor_design_pack", 1)

        routes = [(f"design_B{B}", (lambda B=B: design(B))) for B in BS] + [(f"loop_B{B}", (lambda B=B: loop(B))) for B in BS]
        routes += [(f"loop_rows_in_place_B{B}", (lambda B=B: loop_in_place(B))) for B in (10, 100)]
        routes += [("ten_picks_update_apply_argmax", ten_picks), ("features", features)]
        res = race(routes, args.reps)
        res["in_place_ms_per_step"] = (res["loop_rows_in_place_B100"]["event_ms"] - res["loop_rows_in_place_B10"]["event_ms"]) / 90.0
        res["packed_ms_per_step_B10_to_100"] = (res["loop_B100"]["event_ms"] - res["loop_B10"]["event_ms"]) / 90.0
        res["loop_ms_per_step"] = (res["loop_B1000"]["event_ms"] - res["loop_B100"]["event_ms"]) / 900.0
        res["old_route_ms_per_pick"] = res["ten_picks_update_apply_argmax"]["event_ms"] / 10.0
        for B in BS:
            res[f"old_route_over_design_B{B}"] = res["old_route_ms_per_pick"] * B / res[f"design_B{B}"]["event_ms"]
        res["features_array_bytes"] = 8 * pool * K
        res["design_workspace_bytes"] = {str(B): int(need[B]) for B in BS}
        res["pool_rows_bytes"] = 12 * pool * r
        out["pools"][str(pool)] = res
        print(json.dumps({str(pool): res}, indent=1), flush=True)
        del dX, d_idx, d_val, score, var, work, Z
    src.free(); model.free(); pair.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
