"""Timing of the predictive negative log likelihood (flgp_negative_log_likelihood) on synthetic mean / cov /
target at BASELINE configs[2]'s number of new rows, against a vectorised numpy restatement of the reference's route
(src/Utils.cpp:302-336: n x n_samples normals, four n x n_samples temporaries, exp) on the same machine, OMP_NUM_THREADS
as set.  Rows:

  n = 999 000, J = 1,  n_samples = 100, "binary"
  n = 999 000, J = 10, n_samples = 100, "multinomial"
  n = 999 000,                          "regression"
  n = 1000,    J = 1,  n_samples = 100, "binary"

Per row: call_ms, the host-pointer entry (upload of mean / cov / target included), best and median of --reps calls after
one warm-up; kernel_ms, the sampling (or elementwise) kernel alone by HIP events (flgp_prof); resident_ms, the
device-pointer entry on arrays that are already on the device, synchronised; host_ms, the numpy route in chunks of
--chunk rows so that its temporaries fit in host memory, best of --host-reps.  Prints one JSON object.

Usage: python scripts/time_nll.py [--reps 5] [--host-reps 1] [--chunk 100000]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from flgp_amd import _lib, api  # noqa: E402


def prof(name):
    c = ctypes.c_int(); ms = ctypes.c_double(); w = ctypes.c_double()
    _lib.lib().flgp_prof_query(name.encode(), ctypes.addressof(c), ctypes.addressof(ms), ctypes.addressof(w))
    return c.value, ms.value


def best(fn, reps, warm=True):
    if warm:
        fn()
    ts = []
    out = None
    for _ in range(reps):
        t0 = time.perf_counter(); out = fn(); ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3, float(np.median(ts)) * 1e3, out


def kernel_ms(fn, name):
    L = _lib.lib()
    L.flgp_prof_reset(); L.flgp_prof_enable(2)
    fn()
    torch.cuda.synchronize(); L.flgp_prof_enable(0)
    c, ms = prof(name)
    return ms / max(c, 1)


def host_class(mean, cov, y01, n_samples, rng, chunk):
    """nll_classification as the reference writes it, in chunks of rows"""
    acc = 0.0
    for a in range(0, mean.size, chunk):
        m, c, y = mean[a:a + chunk], cov[a:a + chunk], y01[a:a + chunk]
        f = rng.standard_normal((m.size, n_samples)) * np.sqrt(c)[:, None]
        f += m[:, None]
        pi = 1.0 / (1.0 + np.exp(-f))
        like = (pi * y[:, None] + (1.0 - pi) * (1.0 - y[:, None])).mean(axis=1)
        acc += np.log(like + 1e-2).sum()
    return -acc / mean.size


def host_nll(mean, cov, target, type, n_samples, chunk):
    rng = np.random.default_rng(1)
    if type == "regression":
        return (((target - mean) ** 2 / cov + np.log(cov + 1e-9)).mean() + np.log(2 * 3.1415926)) / 2
    if type == "binary":
        return host_class(mean, cov, target, n_samples, rng, chunk)
    aug = api.multi_train_split(target)
    return sum(host_class(mean[:, j], cov[:, j], aug[:, j], n_samples, rng, chunk) for j in range(aug.shape[1]))


def resident(mean, cov, target, type, n_samples, J):
    """the device-pointer entry on torch tensors: a callable that runs one synchronised call and returns the value"""
    L = _lib.lib()
    n = target.size
    dm, dc, dt = (torch.tensor(np.asfortranarray(a).ravel(order="F"), dtype=torch.float64, device="cuda") for a in (mean, cov, target))
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    work = torch.zeros(L.flgp_dev_nll_workspace(n, J) // 8, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call():
        if type == "regression":
            _lib.check(L.flgp_dev_nll_regression(st, dm.data_ptr(), dc.data_ptr(), dt.data_ptr(), n, None, out.data_ptr(),
                                                 work.data_ptr()))
        else:
            _lib.check(L.flgp_dev_nll_classification(st, dm.data_ptr(), dc.data_ptr(), dt.data_ptr(), n, J,
                                                     int(type == "multinomial"), n_samples, 1, 0, None, out.data_ptr(),
                                                     work.data_ptr()))
        torch.cuda.synchronize()
        return float(out.cpu()[0])
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=100_000)
    args = ap.parse_args()
    torch.cuda.init()       # torch's HIP runtime opens the device before libflgp_hip.so does
    rng = np.random.default_rng(0)
    res = {"reps": args.reps, "host_reps": args.host_reps, "chunk": args.chunk, "threads": os.environ.get("OMP_NUM_THREADS"),
           "rows": []}
    for n, J, ns, type in ((999_000, 1, 100, "binary"), (999_000, 10, 100, "multinomial"), (999_000, 1, 100, "regression"),
                           (1000, 1, 100, "binary")):
        shape = (n, J) if type == "multinomial" else (n,)
        mean = np.asfortranarray(3.0 * rng.standard_normal(shape))
        cov = np.asfortranarray(rng.uniform(0.05, 4.0, shape) ** 2)
        if type == "regression":
            target = mean + np.sqrt(cov) * rng.standard_normal(n)
        elif type == "binary":
            target = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-mean))).astype(np.float64)
        else:
            target = rng.integers(0, J, n).astype(np.float64)
        row = {"n": n, "J": J, "n_samples": ns if type != "regression" else None, "type": type}

        def call():
            return api.negative_log_likelihood(mean, cov, target, type, n_samples=ns, seed=1)
        row["call_ms"], row["call_median_ms"], row["value"] = best(call, args.reps)
        row["kernel_ms"] = kernel_ms(call, "nll_reg_kernel" if type == "regression" else "nll_class_kernel")
        row["resident_ms"], row["resident_median_ms"], v = best(resident(mean, cov, target, type, ns, J), args.reps)
        assert v == row["value"], (v, row["value"])
        row["host_ms"], _, row["host_value"] = best(lambda: host_nll(mean, cov, target, type, ns, args.chunk), args.host_reps,
                                                    warm=False)
        row["speedup_call"] = row["host_ms"] / row["call_ms"]
        res["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
