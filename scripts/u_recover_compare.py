"""GPU box: flgp_dev_u_recover of this tree against the same entry of other builds of the library (the parent commit's,
or variants of the kernel under trial), on the flagship inputs: BASELINE configs[2], all 1e6 rows, through k-NN -> LAE ->
Laplacian scalings -> Gram -> top-K eigenpairs as pipeline.py runs them.  The vectors must be the same bits
(torch.equal); the calls are timed in turn, two rounds after one unrecorded round (HIP events, mean of --reps; the call
is the slice transpose plus the kernel).
usage: python scripts/u_recover_compare.py --other parent=path/to/libflgp_hip.so [--other label=path ...] [--out file.json]"""
import argparse, ctypes, json, math, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flgp_amd import _lib, synth
from flgp_amd.pipeline import HeatKernelPath, HipStages

ap = argparse.ArgumentParser()
ap.add_argument("--other", action="append", required=True, help="label=path")
ap.add_argument("--s", type=int, default=5000)
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--d", type=int, default=16)
ap.add_argument("--r", type=int, default=10)
ap.add_argument("--K", type=int, default=200)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()

S = HipStages("cuda:0")
path = HeatKernelPath(S)
libs = {"this_tree": S.L}
for spec in args.other:
    label, p = spec.split("=", 1)
    L = ctypes.CDLL(os.path.abspath(p))
    for name in ("flgp_dev_u_recover", "flgp_dev_u_recover_workspace"):
        getattr(L, name).restype, getattr(L, name).argtypes = _lib._SIGNATURES[name]
    L.flgp_set_device.argtypes = [ctypes.c_int]
    L.flgp_set_device(0)
    libs[label] = L

n, d, r, s, K = args.n, args.d, args.r, args.s, args.K
X_np = synth.gaussian_mixture(n, d)
X = torch.from_numpy(np.ascontiguousarray(X_np.T)).cuda()
sel = np.sort(synth.random_anchor_rows(n, s))
U = torch.from_numpy(np.ascontiguousarray(X_np[sel].T)).cuda()
A = S.anchor_prep(U)
num_class = path.cluster_sizes(X, A)
knn_idx, _ = S.knn(X, A, r)
ei, ev = S.lae(X, A, knn_idx)
csc = S.csc(ei, s)
S.col_scale_row_normalize(ei, ev, S.colsum(ei, ev, s), num_class)
S.col_scale(ei, ev, S.colsum(ei, ev, s), None, 1)
eig, V, info = S.eig_topk(S.gram(ei, ev, csc), K)
work = S.empty((max(L.flgp_dev_u_recover_workspace(s, K) for L in libs.values()) // 8 + 1,))
scale = math.sqrt(float(n))


def run(L):
    out = torch.full((K, n), float("nan"), dtype=torch.float64, device="cuda:0")
    call = lambda: L.flgp_dev_u_recover(S._st(), ei.data_ptr(), ev.data_ptr(), n, r, V.data_ptr(), s, s, eig.data_ptr(), K, scale,
                                        0, out.data_ptr(), n, None, work.data_ptr())
    for _ in range(3):
        assert call() == 0
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(torch.cuda.current_stream())
    for _ in range(args.reps):
        call()
    e1.record(torch.cuda.current_stream())
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1) / args.reps


ms = {label: [] for label in libs}
equal = {}
ref = None
for rnd in range(3):                                   # round 0 warms every library (and the clocks) up and is not recorded
    for label, L in libs.items():
        out, t = run(L)
        if rnd == 0:
            del out
            continue
        ms[label].append(t)
        if ref is None:
            ref = out
        else:
            equal[label] = equal.get(label, True) and bool(torch.equal(out, ref))
            del out
res = {"n": n, "s": s, "r": r, "K": K, "route": S.L.flgp_dev_u_recover_route(n, r, s, K, 1), "finite": bool(torch.isfinite(ref).all()),
       "equal_to_this_tree": equal, "ms": ms}
print(json.dumps(res), flush=True)
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)
sys.exit(0 if res["finite"] and all(equal.values()) else 1)
