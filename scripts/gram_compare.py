"""GPU box: Gram of this tree (flgp_dev_gram_ordered on the list of flgp_dev_gram_order, as the path runs it; the list's own
kernel is timed beside it) against flgp_dev_gram of another build of the library (the parent commit's), on
the flagship inputs: BASELINE configs[2], all 1e6 rows, through k-NN -> LAE -> Laplacian scalings as pipeline.py runs them.
G must be the same bits (torch.equal); both calls are timed back to back (HIP events, mean of --reps).
usage: python scripts/gram_compare.py --other path/to/libflgp_hip.so [--s 5000 20500] [--n 1000000] [--r 10] [--out file.json]"""
import argparse, ctypes, json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flgp_amd import _lib, synth
from flgp_amd.pipeline import HeatKernelPath, HipStages

ap = argparse.ArgumentParser()
ap.add_argument("--other", required=True)
ap.add_argument("--s", type=int, nargs="+", default=[5000, 20500])      # 20500 > 20000: the kernel works by windows
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--d", type=int, default=16)
ap.add_argument("--r", type=int, default=10)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()

S = HipStages("cuda:0")
path = HeatKernelPath(S)
other = ctypes.CDLL(os.path.abspath(args.other))
P = ctypes.c_void_p
other.flgp_dev_gram.restype = ctypes.c_int
other.flgp_dev_gram.argtypes = _lib._SIGNATURES["flgp_dev_gram"][1]
other.flgp_set_device.argtypes = [ctypes.c_int]
other.flgp_set_device(0)

n, d, r = args.n, args.d, args.r
X_np = synth.gaussian_mixture(n, d)
X = torch.from_numpy(np.ascontiguousarray(X_np.T)).cuda()
results = []
for s in args.s:
    sel = np.sort(synth.random_anchor_rows(n, s))
    U = torch.from_numpy(np.ascontiguousarray(X_np[sel].T)).cuda()
    A = S.anchor_prep(U)
    num_class = path.cluster_sizes(X, A)
    knn_idx, _ = S.knn(X, A, r)
    ei, ev = S.lae(X, A, knn_idx)
    csc = S.csc(ei, s)
    S.col_scale_row_normalize(ei, ev, S.colsum(ei, ev, s), num_class)
    S.col_scale(ei, ev, S.colsum(ei, ev, s), None, 1)
    counts = torch.diff(csc["colptr"]).cpu().numpy()

    def timed(call):
        for _ in range(3):
            assert call() == 0
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream())
        for _ in range(args.reps):
            call()
        e1.record(torch.cuda.current_stream())
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    def run(L, rec_ptr=None):
        G = torch.full((s, s), float("nan"), dtype=torch.float64, device="cuda:0")
        if L is other:
            call = lambda: L.flgp_dev_gram(S._st(), ei.data_ptr(), ev.data_ptr(), n, s, r, csc["colptr"].data_ptr(),
                                           csc["pos"].data_ptr(), G.data_ptr(), s)
        else:
            call = lambda: L.flgp_dev_gram_ordered(S._st(), ei.data_ptr(), ev.data_ptr(), n, s, r, csc["colptr"].data_ptr(),
                                                   csc["pos"].data_ptr(), csc["order"].data_ptr(), rec_ptr, G.data_ptr(), s)
        return G, timed(call)

    order2 = torch.empty_like(csc["order"])
    order_call = lambda: S.L.flgp_dev_gram_order(S._st(), csc["colptr"].data_ptr(), s, order2.data_ptr())
    ms_order = timed(order_call)
    rec = torch.empty((S.L.flgp_dev_gram_record_bytes(n, r) // 8,), dtype=torch.float64, device="cuda:0")
    pack_call = lambda: S.L.flgp_dev_gram_pack(S._st(), ei.data_ptr(), ev.data_ptr(), n, r, rec.data_ptr())
    ms_pack = timed(pack_call)
    G_new, ms_new = run(S.L)
    G_rec, ms_rec = run(S.L, rec.data_ptr())
    G_old, ms_old = run(other)
    G_new2, ms_new2 = run(S.L)
    G_old2, ms_old2 = run(other)
    G_rec2, ms_rec2 = run(S.L, rec.data_ptr())
    ms_pack2 = timed(pack_call)
    ms_order2 = timed(order_call)
    assert torch.equal(order2, csc["order"])
    res = {"n": n, "s": s, "r": r, "equal": bool(torch.equal(G_new, G_old)), "symmetric": bool(torch.equal(G_new, G_new.t())),
           "finite": bool(torch.isfinite(G_new).all()), "ms_this_tree": [ms_new, ms_new2], "ms_other": [ms_old, ms_old2],
           "ms_order_kernel": [ms_order, ms_order2], "ms_from_records": [ms_rec, ms_rec2], "ms_pack_kernel": [ms_pack, ms_pack2],
           "records_equal": bool(torch.equal(G_rec, G_old) and torch.equal(G_rec2, G_old)),
           "column_counts": {"min": int(counts.min()), "median": float(np.median(counts)), "mean": float(counts.mean()),
                             "p99": float(np.percentile(counts, 99)), "max": int(counts.max())}}
    print(json.dumps(res), flush=True)
    results.append(res)
    del G_new, G_old, G_new2, G_old2, G_rec, G_rec2, rec, ei, ev, csc, knn_idx
    torch.cuda.empty_cache()
if args.out:
    json.dump(results, open(args.out, "w"), indent=1)
sys.exit(0 if all(x["equal"] and x["symmetric"] and x["finite"] for x in results) else 1)
