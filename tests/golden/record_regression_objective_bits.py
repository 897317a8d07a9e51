"""Records tests/golden/regression_objective_bits.npz: the bits flgp_eigenpair_regression_objective returns for every
pinned case of tests/regression_objective_cases.py.

DEVICE-RECORDED, not restatement-derived: the fixture is what the library computed on an MI355X at the commit stored in
it -- the last one at which the single entry ran its own steps (RgEval::woodbury_terms for m > K, RgEval::begin and
direct_terms for m <= K), the independent implementation the batch entry was written against.  Re-recording at a later
commit would pin the batch route to itself, so the file is only to be regenerated from a checkout of that commit.

    python tests/golden/record_regression_objective_bits.py --commit $(git rev-parse HEAD) [--out FILE]

Every case runs twice and nothing is written if the two runs differ in any byte.  Stored: keys (the cases' and then the
failures' keys, in table order) and, per key, value_bits and value_only_bits (the uint64 patterns of the value returned
with the gradient and value-only), grad_bits (ragged: one concatenated uint64 array) with grad_offsets (len(keys) + 1),
code and message (0 and "" where the call returned numbers; a failure that is refused stores its return code and exact
text, and NaN patterns with an empty gradient); commit and hip (torch.version.hip) for the record.
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

import regression_objective_cases as C  # noqa: E402


def record(pairs):
    """one pass over the table: [(code, message, value bits, value-only bits, gradient bits)]"""
    out = []
    for c in C.CASES:
        v, v0, g = C.run_single(pairs, c)
        out.append((0, "", C.bits(v), C.bits(v0), C.bits(g)))
    for f in C.FAILURES:
        code, msg, v, v0, g = C.run_failure(f)
        out.append((code, msg, C.bits(v), C.bits(v0), C.bits(g)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit recorded from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=C.BITS_FILE)
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], check=True, capture_output=True,
                                           text=True).stdout.strip()
    torch.cuda.init()       # torch's HIP runtime opens the device before libflgp_hip.so does
    pairs = C.synthetic_pairs()
    first, second = record(pairs), record(pairs)                  # a value that is not reproducible cannot be pinned
    for _, _, rp in pairs:
        rp.free()
    keys = [c.key for c in C.CASES + C.FAILURES]
    for k, a, b in zip(keys, first, second):
        if a[:2] != b[:2] or any(x.tobytes() != y.tobytes() for x, y in zip(a[2:], b[2:])):
            sys.exit(f"{k}: two runs differ; nothing written")
        print(k, a[0], a[1], a[2].view(np.float64)[0], a[4].size, flush=True)
    grads = [a[4] for a in first]
    np.savez_compressed(args.out, keys=np.array(keys), value_bits=np.concatenate([a[2] for a in first]),
                        value_only_bits=np.concatenate([a[3] for a in first]), grad_bits=np.concatenate(grads),
                        grad_offsets=np.concatenate([[0], np.cumsum([g.size for g in grads])]).astype(np.int64),
                        code=np.array([a[0] for a in first], dtype=np.int32), message=np.array([a[1] for a in first]),
                        commit=np.array(commit), hip=np.array(str(torch.version.hip)))
    print("wrote", args.out, os.path.getsize(args.out), "bytes,", len(keys), "keys,", sum(g.size for g in grads), "gradient entries")


if __name__ == "__main__":
    main()
