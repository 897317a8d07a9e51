"""Timing of the Polya-Gamma Gibbs prediction at BASELINE configs[2]'s shape: n = 1e6, K = 200, m = 1000,
m_new = 999 000, N_sample = 100, on a synthetic resident pair.  Prints one JSON object with

  * woodbury: the binary chain on the resident pair (m > K: the K x K Woodbury system), wall time of the whole call at
    N_sample = 100 and N_sample = 1; their difference / 99 is the time of one sweep, the N_sample = 1 call less one sweep
    the setup and the collapsed prediction of the 999 000 new rows;
  * mxm: the m x m route, once on the resident pair with m = K = 200 and once through the dense entry
    (flgp_pg_logit_predict, test_pgbinary_cpp's host matrices) at m = 1000;
  * multiclass: predict_logit_mult_gp_cpp with J = 10 classes (ten chains one after another) at the full shape;
  * reference: a numpy restatement of _resample_f (src/PGLogitModel.cpp:25-39: B, its LLT solve, Sigma = C - ..., its LLT,
    the product with a normal) at m = 1000 with LAPACK, timed over a few sweeps and scaled to 100 sweeps and to 10 classes
    (labelled as scaled).  The pgdraw call of each sweep is left out of the reference's figure.

Usage: python scripts/time_pg_predict.py [--reps 3] [--ref-sweeps 3]
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

from flgp_amd import api  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-sweeps", type=int, default=3)
    args = ap.parse_args()
    torch.cuda.init()
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
    res["multiclass"] = {"call_ms": 1e3 * mc, "per_class_ms": 1e3 * mc / J, "chains": "one after another on one stream"}

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
