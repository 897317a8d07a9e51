"""Timing of the GLGP bandwidth grid (reference src/Fit.cpp:383-449) on device-resident points: the default
ten-point grid of R/Fit.R:227-240, sparse (threshold 0.01) and dense, at n = 5000 and n = 20000, d = 16, K = 100.

Per route and size:
  * every bandwidth as a grid of its own (l = 1), so that one that the eigensolver refuses hides no other: HIP events
    around the call, one warm-up, best of --reps; whether it converged, the library's message if not, the eigensolver's
    outer iterations; and, from one more call with the library's per-stage events on (a run of its own: the events cost
    time), the stages: distances, selection, similarity + normalisations, eigensolve, final scaling;
  * the whole grid in one call (l = 10, max_parallel = 4), if every bandwidth converged alone;
  * the selection stage's achieved bytes/s over one read of the 8 n^2-byte lists (it reads them seven times, six of them
    from cache at best: see DESIGN);
  * for comparison one bandwidth of the restatement on the host: scipy.sparse.linalg.eigsh on the same W (sparse matrix /
    dense array), with as many threads as OMP_NUM_THREADS says (16 for the recorded table).

Writes profiles/glgp_grid_timing.json (or --out) and prints it.

Usage: python scripts/time_glgp_grid.py [--sizes 5000,20000] [--reps 5] [--host-dense-max 5000]
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

from flgp_amd import _lib  # noqa: E402

A2S = np.exp(np.linspace(np.log(0.1), np.log(10.0), 10))
STAGES = ("glgp_distances", "glgp_select", "glgp_similarity_norm", "glgp_eigensolve", "glgp_final")


def timed_call(fn):
    """(rc, ms) of a synchronous library call between two HIP events"""
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(); rc = fn(); e1.record()
    torch.cuda.synchronize()
    return rc, e0.elapsed_time(e1)


def stage_times(L):
    out = {}
    for name in STAGES:
        cnt = ctypes.c_int(); ms = ctypes.c_double(); work = ctypes.c_double()
        if L.flgp_prof_query(name.encode(), ctypes.byref(cnt), ctypes.byref(ms), ctypes.byref(work)) == 0 and cnt.value:
            out[name] = {"ms": ms.value, "launches": cnt.value}
    return out


def device_route(L, X, n, d, K, sparse, thr, reps):
    st = torch.cuda.current_stream().cuda_stream
    val = torch.empty((A2S.size, K), device="cuda", dtype=torch.float64)
    vec = torch.empty((A2S.size, K, n), device="cuda", dtype=torch.float64)
    mean = ctypes.c_double(); r = ctypes.c_int()

    def call(a2s, max_parallel):
        a = np.ascontiguousarray(a2s, dtype=np.float64)
        return L.flgp_dev_glgp_spectrum_grid(st, X.data_ptr(), n, n, d, K, a.ctypes.data, a.size, int(sparse), thr, max_parallel,
                                             val.data_ptr(), vec.data_ptr(), ctypes.byref(mean), ctypes.byref(r))

    per = []
    for a2 in A2S:
        rc, warm = timed_call(lambda: call([a2], 1))
        rec = {"a2": float(a2), "converged": rc == 0, "warmup_ms": warm}
        if rc != 0:
            rec["message"] = L.flgp_last_error().decode("utf-8", "replace")
        it = ctypes.c_int(-1)
        L.flgp_glgp_last_iterations(ctypes.byref(it), 1)
        rec["outer_iterations"] = it.value
        used = reps if warm < 10_000 else 1          # a call of ten seconds and more is timed once
        rec["reps"] = used
        rec["best_ms"] = min(timed_call(lambda: call([a2], 1))[1] for _ in range(used))
        L.flgp_prof_reset(); L.flgp_prof_enable(2)
        _, rec["ms_with_stage_events"] = timed_call(lambda: call([a2], 1))
        L.flgp_prof_enable(0)
        rec["stages"] = stage_times(L)
        L.flgp_prof_reset()
        per.append(rec)
        print(f"n={n} {'sparse' if sparse else 'dense'} a2={a2:.4g}: converged={rec['converged']} iterations={rec['outer_iterations']} "
              f"best {rec['best_ms']:.1f} ms", file=sys.stderr, flush=True)
    out = {"per_bandwidth": per, "r": r.value, "distances_mean": mean.value}
    if all(p["converged"] for p in per):
        rc, warm = timed_call(lambda: call(A2S, 4))
        out["grid_l10_workers4_best_ms"] = min(timed_call(lambda: call(A2S, 4))[1] for _ in range(reps if warm < 30_000 else 1))
        out["grid_l10_one_by_one_sum_ms"] = sum(p["best_ms"] for p in per)
    else:
        rc, _ = timed_call(lambda: call(A2S, 4))
        out["grid_l10"] = "fails: " + L.flgp_last_error().decode("utf-8", "replace") if rc else "converged as a whole"
    sel = [p["stages"]["glgp_select"]["ms"] for p in per if "glgp_select" in p.get("stages", {})]
    if sel:
        out["select_best_ms"] = min(sel)
        out["select_GBps_over_one_read_of_the_lists"] = 8.0 * n * n / (min(sel) * 1e-3) / 1e9
    return out


def host_bandwidth(Xh, K, a2, sparse, thr):
    """one bandwidth of the restatement with scipy's eigsh; the time of the similarity and of the eigensolve"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as sla
    n = Xh.shape[0]
    t0 = time.perf_counter()
    xx = (Xh * Xh).sum(axis=1)
    D = (xx[:, None] - 2.0 * (Xh @ Xh.T)) + xx[None, :]          # row i = list i
    if sparse:
        r = max(int(np.floor(thr * n + 0.5)), 3)
        idx = np.argpartition(D, r - 1, axis=1)[:, :r]
        dist = np.take_along_axis(D, idx, axis=1)
        del D
        mean = dist.mean()
        Z = sp.csr_matrix((np.exp(-dist / (a2 * mean)).ravel(), idx.ravel(), np.arange(0, n * r + 1, r)), shape=(n, n))
        Z = (Z + Z.T) * 0.5
        rs = 1.0 / (np.asarray(Z.sum(axis=1)).ravel() + 1e-9)
        A = sp.diags(rs) @ Z @ sp.diags(rs)
        sd = 1.0 / np.sqrt(np.asarray(A.sum(axis=1)).ravel() + 1e-9)
        W = (sp.diags(sd) @ A @ sp.diags(sd)).tocsr()
    else:
        mean = D.mean()
        np.multiply(D, -1.0 / (a2 * mean), out=D); np.exp(D, out=D)
        rs = 1.0 / (D.sum(axis=1) + 1e-9)
        D *= rs[:, None]; D *= rs[None, :]
        sd = 1.0 / np.sqrt(D.sum(axis=1) + 1e-9)
        D *= sd[:, None]; D *= sd[None, :]
        W = D
    t1 = time.perf_counter()
    vals = sla.eigsh(W, k=K, which="LA", return_eigenvectors=True)[0]
    t2 = time.perf_counter()
    return {"a2": float(a2), "similarity_s": t1 - t0, "eigsh_s": t2 - t1, "lambda_top": float(vals.max()), "lambda_K": float(vals.min()),
            "threads": os.environ.get("OMP_NUM_THREADS", "unset")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5000,20000")
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.01)
    ap.add_argument("--host-a2-index", type=int, default=5)
    ap.add_argument("--host-dense-max", type=int, default=5000, help="largest n whose dense host comparison is run")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glgp_grid_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_glgp_grid.py needs the GPU: nothing here is measured without one")
    torch.cuda.init()       # torch's HIP runtime opens the device before libflgp_hip.so does
    L = _lib.lib()
    res = {"a2s": A2S.tolist(), "d": args.d, "K": args.K, "threshold": args.threshold, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "sizes": {}}
    for n in (int(v) for v in args.sizes.split(",")):
        gen = torch.Generator(device="cuda").manual_seed(n + args.d)
        X = torch.randn((args.d, n), generator=gen, device="cuda", dtype=torch.float64)      # column-major n x d
        entry = {}
        for name, sparse in (("sparse", True), ("dense", False)):
            entry[name] = device_route(L, X, n, args.d, args.K, sparse, args.threshold, args.reps)
            if args.no_host:
                entry[name]["host"] = "not measured"
            elif sparse or n <= args.host_dense_max:
                entry[name]["host"] = host_bandwidth(X.cpu().numpy().T.copy(), args.K, A2S[args.host_a2_index], sparse, args.threshold)
            else:
                entry[name]["host"] = "not measured"
            res["sizes"][str(n)] = entry
            with open(args.out, "w") as f:          # after every route: a later one that runs long loses nothing
                json.dump(res, f, indent=1)
        del X
        torch.cuda.empty_cache()
        L.flgp_dev_pool_release()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
