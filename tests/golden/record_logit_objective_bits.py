"""Records tests/golden/logit_objective_bits.npz: the bits flgp_eigenpair_logit_objective returns for every pinned case of
tests/logit_objective_cases.py.

DEVICE-RECORDED, not restatement-derived: the fixture is what the library computed on an MI355X at the commit stored in
it -- the last one at which the single entry ran its own Newton loops (GpcLowRank for m > K, hk_c11 + logit_la_on_device
for m <= K), the independent implementation the batch entry was written against.  Re-recording at a later commit would
pin the batch route to itself, so the file is only to be regenerated from a checkout of that commit.

    python tests/golden/record_logit_objective_bits.py --commit $(git rev-parse HEAD) [--out FILE]

Stored: keys (the group keys, in table order), and per problem group (index into keys), col, t, bits (the value's
uint64 bit pattern) and iters (int32); commit and hip (torch.version.hip) for the record.
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

import logit_objective_cases as C  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit recorded from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=C.BITS_FILE)
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], check=True, capture_output=True,
                                           text=True).stdout.strip()
    torch.cuda.init()       # torch's HIP runtime opens the device before libflgp_hip.so does
    _, rp = C.synthetic_pair(C.N_ROWS, C.N_COLS, C.PAIR_SEED)
    group, col, t, bits, iters = [], [], [], [], []
    for i, g in enumerate(C.GROUPS):
        cols, ts = C.problems(g)
        v, it = C.run_single(rp, g)
        v2, it2 = C.run_single(rp, g)                              # a value that is not reproducible cannot be pinned
        assert v.tobytes() == v2.tobytes() and np.array_equal(it, it2), g.key
        group += [i] * len(cols); col += cols.tolist(); t += ts.tolist()
        bits += v.view(np.uint64).tolist(); iters += it.tolist()
        print(g.key, it.tolist(), flush=True)
    rp.free()
    np.savez_compressed(args.out, keys=np.array([g.key for g in C.GROUPS]), group=np.array(group, dtype=np.int32),
                        col=np.array(col, dtype=np.int32), t=np.array(t, dtype=np.float64),
                        bits=np.array(bits, dtype=np.uint64), iters=np.array(iters, dtype=np.int32),
                        commit=np.array(commit), hip=np.array(str(torch.version.hip)))
    print("wrote", args.out, len(bits), "problems in", len(C.GROUPS), "groups")


if __name__ == "__main__":
    main()
