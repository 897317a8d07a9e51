"""CPU: the pinned cases of the Polya-Gamma prediction (pg_predict_cases.CASES) cover what they are meant to, and the
device-recorded fixture tests/golden/pg_predict_bits.npz is the one of this table and stays a small file."""
import os
import re

import numpy as np

import pg_predict_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the panel width of chol_blocked / lrb_chol
CNB = int(re.search(r"constexpr int CNB = (\d+);", open(os.path.join(ROOT, "flgp_amd", "csrc", "gpc.hip")).read()).group(1))


def test_the_table_covers_both_routes_every_edge_and_both_sigma_nv():
    keys = [c.key for c in C.CASES]
    assert len(set(keys)) == len(keys)
    binary = [c for c in C.CASES if c.entry == "binary"]
    assert {(c.K, c.m, c.sigma_nv) for c in binary} == {(K, m, s) for K, m in C.SHAPES for s in C.SIGMA_NVS}
    assert len(binary) == 2 * len(C.SHAPES) and 0.0 in C.SIGMA_NVS and any(s != 0.0 for s in C.SIGMA_NVS)
    shapes = C.SHAPES
    assert any(m < K for K, m in shapes) and any(m == K for K, m in shapes) and any(m == K + 1 for K, m in shapes)
    assert any(m > K and m > 256 and m % 32 != 0 for K, m in shapes)       # a second 256-thread block, padded slot strides
    assert any(m > K and K % 32 != 0 and K > 32 for K, m in shapes)        # K no multiple of 32
    assert (CNB + 1, CNB + 2) in shapes                                    # one column past the Cholesky panel
    assert (16, 48) in shapes
    for c in binary:
        assert c.ts == (1.5, 4.0, 2.25) and c.seed == (11, 2 ** 63 + 5, 2 ** 64 - 1)
        Y = C.responses(c)
        assert Y.shape == (c.m, 3) and set(np.unique(Y[:, :2])) <= {0.0, 1.0}
        assert set(np.unique(Y[:, 2])) <= {0.0, 0.25, 0.75, 1.0} and ((Y[:, 2] > 0) & (Y[:, 2] < 1)).any()      # soft labels
    classes = [c for c in C.CASES if c.entry == "classes"]
    assert [(c.K, c.m, len(c.ts), c.seed) for c in classes] == [(24, 20, 3, 500), (12, 60, 3, 500), (40, 41, 4, 2 ** 64 - 2)]
    assert all(c.ts[:3] == (1.5, 2.5, 4.0) and c.sigma_nv == 0.0 for c in classes)
    wrap = classes[-1]
    assert wrap.seed + len(wrap.ts) - 1 >= 2 ** 64                         # seed + j wraps
    labels = C.class_labels(wrap)
    assert not (labels == 3).any() and all((labels == j).any() for j in range(3))      # class 3 has no member
    # the short idx1, and rows of it among idx0: sigma_nv's match term has entries
    for c in C.CASES:
        idx0, idx1 = C.rows(c)
        assert idx1.size == 39 and idx0.size == c.m == np.unique(idx0).size and idx0.max() < C.N
        assert c.sigma_nv == 0.0 or np.intersect1d(idx0, idx1).size > 0


def test_the_fixture_is_this_tables():
    pinned = C.load_bits()                                        # asserts the keys, the dtypes and the shapes
    assert sorted(pinned) == sorted(c.key for c in C.CASES)
    with np.load(C.BITS_FILE) as z:
        assert len(str(z["commit"])) == 40 and str(z["hip"])
        stored = {k for k in z.files if k not in ("keys", "commit", "hip")}
    assert stored == {f"{k}{i}" for i, c in enumerate(C.CASES) for k in C.out_keys(c)}
    for c in C.CASES:
        p = {k: v.view(np.float64) for k, v in pinned[c.key].items()}
        assert all(np.isfinite(v).all() for v in p.values())
        if c.entry == "binary":
            assert ((p["pi_pred"] > 0) & (p["pi_pred"] < 1)).all() and (p["omega"] > 0).all()
            assert np.array_equal(p["Y_pred"], (p["pi_pred"] > 0.5).astype(float))
        else:
            assert np.array_equal(p["labels"], np.argmax(p["probs"], axis=1).astype(float))
    golden = os.path.dirname(C.BITS_FILE)
    others = [os.path.getsize(os.path.join(golden, f)) for f in os.listdir(golden)
              if os.path.join(golden, f) != C.BITS_FILE and os.path.isfile(os.path.join(golden, f))]
    assert os.path.getsize(C.BITS_FILE) <= max(others)            # no larger than the largest fixture before this one
