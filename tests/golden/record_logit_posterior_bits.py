"""Records tests/golden/logit_posterior_bits.npz: the bits the logit posterior returns for every pinned case of
tests/logit_posterior_cases.py.

DEVICE-RECORDED, not restatement-derived: the fixture is what the library computed on an MI355X at the commit stored in
it -- the last one at which flgp_eigenpair_logit_posterior ran a weight-space Newton loop of its own and
flgp_eigenpair_logit_posterior_multiclass dealt J such loops to a pool of workers, the independent implementations the
batch entry was written against.  Only those two entries are called here (the multiclass one at max_parallel = 1).
Re-recording at a later commit would pin the batch route to itself, so the file is only to be regenerated from a checkout
of that commit.

    python tests/golden/record_logit_posterior_bits.py --commit $(git rev-parse HEAD) [--out FILE]

Stored: keys (the case keys, in table order); per case i mean{i}, cov{i} (uint64 bit patterns, m_new x problems) and
iters{i} (int32); code and message per case (0 and "" where the call succeeds); commit and hip (torch.version.hip) for the
record.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

import logit_posterior_cases as C  # noqa: E402


def run(pairs, c):
    return C.run_binary(pairs(c), c) if c.entry == "binary" else C.run_classes(pairs(c), c, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit recorded from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=C.BITS_FILE)
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], check=True, capture_output=True,
                                           text=True).stdout.strip()
    torch.cuda.init()       # torch's HIP runtime opens the device before libflgp_hip.so does
    pairs = C.Pairs()
    arrays, code, message = {}, [], []
    for i, c in enumerate(C.CASES):
        mean, cov, its, rc, msg = run(pairs, c)
        mean2, cov2, its2, rc2, msg2 = run(pairs, c)               # a value that is not reproducible cannot be pinned
        assert mean.tobytes() == mean2.tobytes() and cov.tobytes() == cov2.tobytes() and np.array_equal(its, its2), c.key
        assert (rc, msg) == (rc2, msg2) and (rc != 0) == c.fails, (c.key, rc, msg)
        arrays[f"mean{i}"] = np.ascontiguousarray(mean).view(np.uint64)
        arrays[f"cov{i}"] = np.ascontiguousarray(cov).view(np.uint64)
        arrays[f"iters{i}"] = its
        code.append(rc); message.append(msg)
        print(c.key, its.tolist(), rc, msg, flush=True)
    pairs.free()
    np.savez_compressed(args.out, keys=np.array([c.key for c in C.CASES]), code=np.array(code, dtype=np.int32),
                        message=np.array(message), commit=np.array(commit), hip=np.array(str(torch.version.hip)), **arrays)
    print("wrote", args.out, os.path.getsize(args.out), "bytes,", len(C.CASES), "cases")


if __name__ == "__main__":
    main()
