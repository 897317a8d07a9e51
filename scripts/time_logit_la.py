"""Timing of the classification consumers at BASELINE configs[2]'s shape: n = 1e6, K = 200, m = 1000,
m_new = 999 000, on a synthetic resident pair.  Prints one JSON object with

  * objective: one marginal-likelihood evaluation on the device (HK(idx, idx) + sigma I built from the resident V, the
    Newton loop, the scalar back) and its Newton iterations; the device time of one iteration (flgp_prof) against its
    wall time, whose difference is the host's per-iteration read-back; and the host route the adapters take today
    (H down, then Alg. 3.1 in numpy with LAPACK potrf per iteration);
  * cholesky: the blocked factorisation alone against the one-workgroup chol_solve_kernel at the same m, and numpy's
    potrf on the host;
  * posterior: posterior_distribution_classification for the 999 000 new rows on the device; the host route (C21 formed,
    C21 beta, Alg. 3.2 as the reference) is timed on a slice of new rows and scaled linearly (labelled as such).

Usage: python scripts/time_logit_la.py [--reps 5] [--slice 20000]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import scipy.linalg as sl

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from flgp_amd import _lib, api  # noqa: E402


def prof(name):
    c = ctypes.c_int(); ms = ctypes.c_double(); w = ctypes.c_double()
    _lib.lib().flgp_prof_query(name.encode(), ctypes.addressof(c), ctypes.addressof(ms), ctypes.addressof(w))
    return c.value, ms.value


def host_newton(C, Y, N, tol=1e-5, max_iter=100):
    m = Y.size
    f = np.zeros(m)
    for it in range(1, max_iter + 1):
        pi = 1.0 / (1.0 + np.exp(-f))
        W = N * pi * (1 - pi)
        sW = np.sqrt(W)
        B = sW[:, None] * C * sW[None, :] + np.eye(m)
        L = sl.cholesky(B, lower=True)                    # LAPACK potrf
        b = W * f + Y * (1 - pi) + (N - Y) * (-pi)
        a = b - sW * sl.cho_solve((L, True), sW * (C @ b))
        f_new = C @ a
        done = np.abs(f - f_new).sum() < tol
        f = f_new
        if done:
            break
    pi = 1.0 / (1.0 + np.exp(-f))
    return -0.5 * (a * f).sum() + (Y * np.log(pi)).sum() + ((N - Y) * np.log(1 - pi)).sum() - np.log(np.diag(L) + 1e-9).sum(), it


def best(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); out = fn(); ts.append(time.perf_counter() - t0)
    return min(ts), float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slice", type=int, default=20000)
    args = ap.parse_args()
    torch.cuda.init()       # torch's HIP runtime opens the device before libflgp_hip.so does
    n, K, m = 1_000_000, 200, 1000
    rng = np.random.default_rng(0)
    values = np.sort(rng.uniform(0.4, 1.0, K))[::-1].copy()
    V = np.asfortranarray(rng.standard_normal((n, K)))
    rp = api.ResidentEigenPair.from_host(api.EigenPair(values, V))
    idx0 = np.arange(m); idx1 = np.arange(m, n)
    Y = (rng.uniform(size=m) < 0.3).astype(np.float64); N = np.ones(m)
    t, sigma = 4.0, 1e-3
    L = _lib.lib()
    res = {"shape": dict(n=n, K=K, m=m, m_new=n - m), "reps": args.reps}

    # objective evaluation
    rp.marginal_log_likelihood_logit_la(K, t, idx0, Y, N, sigma=sigma)      # warm-up
    dev_min, dev_med, (amll, iters) = best(lambda: rp.marginal_log_likelihood_logit_la(K, t, idx0, Y, N, sigma=sigma,
                                                                                       return_iters=True), args.reps)
    L.flgp_prof_reset(); L.flgp_prof_enable(2)
    w0 = time.perf_counter()
    rp.marginal_log_likelihood_logit_la(K, t, idx0, Y, N, sigma=sigma)
    wall_prof = time.perf_counter() - w0
    torch.cuda.synchronize(); L.flgp_prof_enable(0)
    it_count, it_ms = prof("logit_la_newton_iter")
    ch_count, ch_ms = prof("chol_blocked")

    def host_route():
        C = rp.HK_from_spectrum_cpp(K, t, idx0, idx0) + sigma * np.eye(m)    # H down
        return host_newton(C, Y, N)
    host_min, host_med, (amll_h, it_h) = best(host_route, args.reps)
    res["objective"] = dict(device_ms=dev_min * 1e3, device_median_ms=dev_med * 1e3, iterations=iters, amll=amll,
                            host_route_ms=host_min * 1e3, host_route_median_ms=host_med * 1e3, host_iterations=it_h,
                            host_amll=amll_h, speedup=host_min / dev_min,
                            profiled_wall_ms=wall_prof * 1e3,
                            iter_device_ms=it_ms / max(it_count, 1), iter_wall_ms=dev_min * 1e3 / max(iters, 1),
                            chol_in_loop_ms=ch_ms / max(ch_count, 1))

    # the factorisation alone
    x = rng.uniform(-3, 3, size=(m, 2))
    C = 4.0 * np.exp(-0.5 * ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)) + np.eye(m)
    src = torch.tensor(C.T.copy(), device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = {}
    for name, single in (("blocked", 0), ("single_workgroup", 1)):
        times = []
        for r in range(args.reps + 1):
            A = src.clone(); flag.zero_()
            torch.cuda.synchronize()
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(L.flgp_dev_cholesky(None, A.data_ptr(), m, single, flag.data_ptr()))
            e1.record(); torch.cuda.synchronize()
            if r:
                times.append(e0.elapsed_time(e1))
        assert flag.item() == 0
        out[name + "_ms"] = min(times)
        out[name + "_median_ms"] = float(np.median(times))
    h_min, h_med, _ = best(lambda: sl.cholesky(C, lower=True), args.reps)
    out["host_potrf_ms"] = h_min * 1e3
    out["m"] = m
    res["cholesky"] = out

    # posterior for the 999 000 new rows
    rp.posterior_distribution_classification(idx0, idx1[:1000], K, t, Y, sigma, sigma)    # warm-up
    p_min, p_med, post = best(lambda: rp.posterior_distribution_classification(idx0, idx1, K, t, Y, sigma, sigma),
                              max(2, args.reps // 2))
    sl_rows = idx1[:args.slice]
    lam = np.exp(-t * (1.0 - values))

    def host_post():
        C11 = rp.HK_from_spectrum_cpp(K, t, idx0, idx0) + sigma * np.eye(m)
        f = np.zeros(m)
        for _ in range(100):
            pi = 1.0 / (1.0 + np.exp(-f)); W = pi * (1 - pi); sW = np.sqrt(W)
            Lb = sl.cholesky(sW[:, None] * C11 * sW[None, :] + np.eye(m), lower=True)
            b = W * f + (Y - pi)
            a = b - sW * sl.cho_solve((Lb, True), sW * (C11 @ b))
            fn = C11 @ a; done = np.abs(f - fn).sum() < 1e-5; f = fn
            if done:
                break
        pi = 1.0 / (1.0 + np.exp(-f)); sW = np.sqrt(pi * (1 - pi))
        Lb = sl.cholesky(sW[:, None] * C11 * sW[None, :] + np.eye(m), lower=True)
        beta = sW[:, None] * sl.cho_solve((Lb, True), np.eye(m)) * sW[None, :]
        t_fixed = time.perf_counter()
        C21 = rp.HK_from_spectrum_cpp(K, t, sl_rows, idx0)                    # the slice's C21 comes down
        mean = C21 @ (Y - pi)
        C22 = ((V[sl_rows] ** 2) * lam).sum(1) + sigma
        cov = C22 - ((C21 @ beta) * C21).sum(1)
        return t_fixed, mean, cov
    t0 = time.perf_counter(); t_fixed, _, _ = host_post(); t_end = time.perf_counter()
    per_row = (t_end - t_fixed) / sl_rows.size
    res["posterior"] = dict(device_ms=p_min * 1e3, device_median_ms=p_med * 1e3, m_new=idx1.size,
                            host_fixed_ms=(t_fixed - t0) * 1e3, host_slice_rows=int(sl_rows.size),
                            host_slice_ms=(t_end - t_fixed) * 1e3,
                            host_route_extrapolated_ms=((t_fixed - t0) + per_row * idx1.size) * 1e3,
                            min_cov=float(post["cov"].min()))
    rp.free()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
