"""Records tests/golden/pg_predict_bits.npz: the bits the Polya-Gamma prediction returns for every pinned case of
tests/pg_predict_cases.py.

DEVICE-RECORDED, not restatement-derived: the fixture is what the library computed on an MI355X at the commit stored in
it -- the last one at which flgp_eigenpair_pg_predict ran a Woodbury sweep of its own (PgChain's low-rank route) and
flgp_eigenpair_pg_predict_multiclass ran J such chains one after another, the independent implementation the batch entry
was written against.  Only those two entries are called here (test_pgbinary(..., return_state=True) and
predict_logit_mult_gp_cpp(..., output_probs=True)).  Re-recording at a later commit would pin the batch route to itself, so
the file is only ever regenerated from a checkout of that commit: copy this recorder and tests/pg_predict_cases.py
there, build that commit's library and run

    python tests/golden/record_pg_predict_bits.py --commit $(git rev-parse HEAD) [--out FILE]

Stored: keys (the case keys, in table order); per case i the uint64 bit patterns pi_pred{i}, Y_pred{i} (m_new x 3), omega{i},
f{i} (m x 3) of a binary case or probs{i} (m_new x J), labels{i} (m_new) of a class case; commit and hip (torch.version.hip)
for the record.
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

import pg_predict_cases as C  # noqa: E402


def run(pairs, c):
    return C.run_binary(pairs(c), c) if c.entry == "binary" else C.run_classes(pairs(c), c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit recorded from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=C.BITS_FILE)
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], check=True, capture_output=True,
                                           text=True).stdout.strip()
    torch.cuda.init()       # torch's HIP runtime opens the device before libflgp_hip.so does
    pairs = C.Pairs()
    arrays = {}
    for i, c in enumerate(C.CASES):
        a, b = run(pairs, c), run(pairs, c)                        # a value that is not reproducible cannot be pinned
        for k in C.out_keys(c):
            assert a[k].shape == C.out_shape(c, k) and a[k].tobytes(order="F") == b[k].tobytes(order="F"), (c.key, k)
            assert np.isfinite(a[k]).all(), (c.key, k)
            arrays[f"{k}{i}"] = C.bits(a[k])
        print(c.key, "ok", flush=True)
    pairs.free()
    np.savez_compressed(args.out, keys=np.array([c.key for c in C.CASES]), commit=np.array(commit),
                        hip=np.array(str(torch.version.hip)), **arrays)
    print("wrote", args.out, os.path.getsize(args.out), "bytes,", len(C.CASES), "cases")


if __name__ == "__main__":
    main()
