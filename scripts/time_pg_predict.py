"""Timing of the Polya-Gamma Gibbs prediction at BASELINE configs[2]'s shape: n = 1e6, K = 200, m = 1000,
m_new = 999 000, N_sample = 100, on a synthetic resident pair.  Prints one JSON object with

  * woodbury: the binary chain on the resident pair (m > K: the K x K Woodbury system), wall time of the whole call at
    N_sample = 100 and N_sample = 1; their difference / 99 is the time of one sweep, the N_sample = 1 call less one sweep
    the setup and the collapsed prediction of the 999 000 new rows;
  * mxm: the m x m route, once on the resident pair with m = K = 200 and once through the dense entry
    (flgp_pg_logit_predict, test_pgbinary_cpp's host matrices) at m = 1000;
  * multiclass: predict_logit_mult_gp_cpp with J = 10 classes (the batch of ten chains) at the full shape;
  * reference: a numpy restatement of _resample_f (src/PGLogitModel.cpp:25-39: B, its LLT solve, Sigma = C - ..., its LLT,
    the product with a normal) at m = 1000 with LAPACK, timed over a few sweeps and scaled to 100 sweeps and to 10 classes
    (labelled as scaled).  The pgdraw call of each sweep is left out of the reference's figure.

--single: the resident-pair entries alone, wall clock, at the rows of single_rows(); --compare PARENT_LIB: that under the
parent commit's library and this tree's in alternating fresh processes, with the gate of compare()
(profiles/pg_predict_single_timing.json).

Usage: python scripts/time_pg_predict.py [--reps 3] [--ref-sweeps 3]
       python scripts/time_pg_predict.py --compare /path/to/parent/libflgp_hip.so --out profiles/pg_predict_single_timing.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.linalg as sl

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from flgp_amd import _lib, api, synth  # noqa: E402


def best(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return min(ts), float(np.median(ts))


def reference_sweep(C, kappa, omega, rng):
    """_resample_f as the reference writes it (dense, two factorisations, one m^3 product)"""
    m = C.shape[0]
    sw = np.sqrt(omega)
    B = sw[:, None] * C * sw[None, :] + np.eye(m)
    cf = sl.cho_factor(B, lower=True)
    S = C - C @ (sw[:, None] * sl.cho_solve(cf, sw[:, None] * C))
    mu = S @ kappa
    L = sl.cholesky(S, lower=True)
    return mu + L @ rng.standard_normal(m)


def single_rows(reps):
    """--single: the binary, the one-vs-rest and the batch entry at n = 1e6, K = 200, N_sample = 100, m_new = n - m (DESIGN 8
    f-16's shapes; wall clock around the Python call, best of `reps` after a warm-up), and the create of the Polya-Gamma
    predictor of scripts/time_predictor_pg.py (its "model" part: ten chains at m = 1000 on the fitted pair).  {row: ms}"""
    n, K, ns, J, sigma, seed = 1_000_000, 200, 100, 10, 1e-3, 1
    rng = np.random.default_rng(0)
    values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
    V = np.asfortranarray(rng.standard_normal((n, K)) / np.sqrt(K))
    rp = api.ResidentEigenPair.from_host(api.EigenPair(values, V))
    del V
    ts = np.linspace(2.0, 6.0, J)
    out = {}

    def row(name, fn):
        fn()
        out[name] = best(fn, reps)[0] * 1e3

    for m in (1000, 10_000, 200):
        idx0 = np.arange(m); idx1 = np.arange(m, n)
        labels = rng.integers(0, J, m).astype(np.float64)
        y = (labels == 0).astype(np.float64)
        row(f"binary m={m}", lambda: rp.test_pgbinary(idx0, idx1, K, 4.0, y, sigma, 0.0, N_sample=ns, output_pi=True, seed=seed))
        if m == 1000:
            over = np.arange(m // 2, n - m + m // 2)              # m_new = n - m rows, half of idx0 among them
            row("binary m=1000 sigma_nv", lambda: rp.test_pgbinary(idx0, over, K, 4.0, y, sigma, sigma, N_sample=ns, output_pi=True,
                                                                   seed=seed))
            Y = np.asfortranarray((labels[:, None] == np.arange(J)[None, :]).astype(np.float64))
            row("batch B=10 m=1000", lambda: rp.test_pgbinary_batch(idx0, idx1, K, ts, Y, sigma, 0.0, seed=seed, N_sample=ns,
                                                                    output_pi=True))
        row(f"multiclass J=10 m={m}", lambda: rp.predict_logit_mult_gp_cpp(idx0, idx1, K, ts, labels, sigma, N_sample=ns, seed=seed))
    rp.free()
    d, s, r, m = 16, 5000, 10, 1000
    X = synth.gaussian_mixture(n, d)
    U0 = synth.anchors_from_rows(X, np.sort(synth.random_anchor_rows(n, s)))
    sizes = np.bincount(api.KNN_cpp(X, U0, 1)["ind_knn"][:, 0], minlength=s).astype(float)
    U = np.asfortranarray(np.hstack([U0, sizes[:, None]]))
    model, pair = api.heat_kernel_spectrum_model(X, X[:0], s, r, K, models={"kernel": "lae", "gl": "cluster-normalized", "root": True},
                                                 U=U)
    x0 = X[:m, 0]
    labels = np.minimum((np.argsort(np.argsort(x0)) * J) // m, J - 1).astype(np.float64)
    row("pg_create J=10 m=1000", lambda: api.Predictor.pg_for_classes(model, pair, np.arange(m, dtype=np.int32), K, np.full(J, 2.0),
                                                                       labels, 1e-2, N_sample=ns, seed=4242).free())
    model.free(); pair.free()
    return out


def compare(parent_lib, rounds, reps, out_path):
    """--compare: --single under the library of the parent commit and under this tree's, alternating, each round a fresh
    process with its own time limit.  Gate per row: head's best <= parent's best + parent's spread (max -
    min of its rounds)."""
    import subprocess
    runs = {"parent": [], "head": []}
    for _ in range(rounds):
        for who, lib in (("parent", parent_lib), ("head", None)):
            cmd = [sys.executable, os.path.abspath(__file__), "--single", "--reps", str(reps)] + (["--lib", lib] if lib else [])
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=400, check=True)
            runs[who].append(json.loads(res.stdout.strip().splitlines()[-1]))
            print(who, runs[who][-1], file=sys.stderr, flush=True)
    rows = []
    for name in runs["parent"][0]:
        p = [r[name] for r in runs["parent"]]; h = [r[name] for r in runs["head"]]
        rows.append(dict(row=name, parent_rounds_ms=p, head_rounds_ms=h, parent_best_ms=min(p), parent_spread_ms=max(p) - min(p),
                         head_best_ms=min(h), within_gate=bool(min(h) <= min(p) + (max(p) - min(p)))))
    res = {"shape": dict(n=1_000_000, K=200, N_sample=100, m_new="n - m"), "rounds": rounds, "reps": reps, "rows": rows}
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-sweeps", type=int, default=3)
    ap.add_argument("--single", action="store_true", help="time the resident-pair entries alone (see single_rows)")
    ap.add_argument("--lib", default=None, help="with --single: another build of libflgp_hip.so")
    ap.add_argument("--compare", default=None, metavar="PARENT_LIB", help="--single under PARENT_LIB and this tree's library")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.compare:
        return compare(args.compare, args.rounds, args.reps, args.out)
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    torch.cuda.init()
    if args.single:
        print(json.dumps(single_rows(args.reps)))
        return
    n, K, m, ns, J = 1_000_000, 200, 1000, 100, 10
    rng = np.random.default_rng(0)
    values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
    V = np.asfortranarray(rng.standard_normal((n, K)) / np.sqrt(K))
    rp = api.ResidentEigenPair.from_host(api.EigenPair(values, V))
    idx0 = np.arange(m); idx1 = np.arange(m, n)
    Y = (rng.uniform(size=m) < 0.3).astype(np.float64)
    t, sigma = 4.0, 1e-3
    res = {"shape": dict(n=n, K=K, m=m, m_new=n - m, N_sample=ns, J=J), "reps": args.reps}

    def binary(k, i0, i1, y, nsamp):
        return lambda: rp.test_pgbinary(i0, i1, k, t, y, sigma, sigma, N_sample=nsamp, output_pi=True, seed=1)

    binary(K, idx0, idx1, Y, 2)()                     # warm the pool and the code objects
    full, _ = best(binary(K, idx0, idx1, Y, ns), args.reps)
    one, _ = best(binary(K, idx0, idx1, Y, 1), args.reps)
    sweep = (full - one) / (ns - 1)
    res["woodbury"] = {"call_ms": 1e3 * full, "sweep_ms": 1e3 * sweep,
                       "setup_and_prediction_ms": 1e3 * (one - sweep)}

    m2 = K
    i0s = np.arange(m2); Ys = Y[:m2]
    full2, _ = best(binary(K, i0s, idx1, Ys, ns), args.reps)
    one2, _ = best(binary(K, i0s, idx1, Ys, 1), args.reps)
    C = np.asfortranarray(rp.HK_from_spectrum_cpp(K, t, idx0, idx0) + sigma * np.eye(m))
    Cnv = np.asfortranarray(rp.HK_from_spectrum_cpp(K, t, np.arange(m, 2 * m), idx0))
    dfull, _ = best(lambda: api.test_pgbinary_cpp(C, Y, Cnv, N_sample=ns, seed=1), args.reps)
    done, _ = best(lambda: api.test_pgbinary_cpp(C, Y, Cnv, N_sample=1, seed=1), args.reps)
    res["mxm"] = {"resident_m200": {"call_ms": 1e3 * full2, "sweep_ms": 1e3 * (full2 - one2) / (ns - 1)},
                  "dense_m1000": {"call_ms": 1e3 * dfull, "sweep_ms": 1e3 * (dfull - done) / (ns - 1),
                                  "note": "m_new = 1000 rows of Cnv; C and Cnv uploaded by the call"}}

    Yj = rng.integers(0, J, m).astype(np.float64)
    ts = np.linspace(2.0, 6.0, J)
    mc, _ = best(lambda: rp.predict_logit_mult_gp_cpp(idx0, idx1, K, ts, Yj, sigma, N_sample=ns, seed=1), args.reps)
    res["multiclass"] = {"call_ms": 1e3 * mc, "per_class_ms": 1e3 * mc / J, "chains": "the batch of J"}

    kappa = Y - 0.5
    om = np.ones(m)
    r2 = np.random.default_rng(1)
    t0 = time.perf_counter()
    for _ in range(args.ref_sweeps):
        reference_sweep(C, kappa, om, r2)
    ref = (time.perf_counter() - t0) / args.ref_sweeps
    res["reference"] = {"sweep_ms": 1e3 * ref, "binary_100_sweeps_ms_scaled": 1e3 * ref * ns,
                        "multiclass_J10_ms_scaled": 1e3 * ref * ns * J, "threads": os.environ.get("OMP_NUM_THREADS")}
    rp.free()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
