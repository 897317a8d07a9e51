"""CPU: the pinned cases of the logit posterior (logit_posterior_cases.CASES) cover what they are meant to, and the
device-recorded fixture tests/golden/logit_posterior_bits.npz is the one of this table and stays a small file."""
import os

import numpy as np

import logit_posterior_cases as C


def test_the_table_covers_both_routes_every_edge_and_both_sigma_pairs():
    keys = [c.key for c in C.CASES]
    assert len(set(keys)) == len(keys)
    binary = [c for c in C.CASES if c.entry == "binary" and not c.fails]
    plain = [c for c in binary if c.cols == C.COLS4 and c.kind1 == "set"]
    assert {(c.K, c.m, c.sig) for c in plain} == {(K, m, sig) for K, m in C.SHAPES for sig in C.SIGMAS}
    assert {c.kind0 for c in plain} == {"range", "perm"}
    assert any(c.m <= c.K for c in plain) and any(c.m == c.K for c in plain) and any(c.m == c.K + 1 for c in plain)
    # the edges by name: the operand's 16-row tile, a second 256-thread block, a second Cholesky panel, both fused row blocks
    for shape in ((15, 16), (16, 17), (17, 35), (12, 257), (65, 66), (129, 263), (205, 206), (1, 2)):
        assert shape in C.SHAPES
    assert len(set(zip(C.COLS4, C.TS4))) == 4
    assert any(c.kind1 == "range" for c in binary)
    assert sorted(c.max_iter for c in binary if c.cols == C.MIXED_COLS) == [2, 100]
    assert [(c.K, c.m, c.n, len(c.ts)) for c in binary if c.K > 1024] == [C.WIDE + (2,)]
    classes = [c for c in C.CASES if c.entry == "classes" and not c.fails]
    assert {(c.K, c.m, c.sig) for c in classes if len(c.ts) == 5} == {(K, m, sig) for K, m in ((33, 300), (40, 24))
                                                                      for sig in C.SIGMAS}
    for c in classes:
        labels = C.class_labels(c)
        if len(c.ts) == 5:
            assert not (labels == 3).any() and (labels == 4).any()         # a class without a member
    assert [(c.K, len(c.ts)) for c in classes if len(c.ts) != 5] == [(64, 10)]
    assert sorted(c.entry for c in C.CASES if c.fails) == ["binary", "classes"]
    # the short idx1: an index set over one full 32-row block and a partial one
    idx1 = C.rows1("set")
    assert 32 < idx1.size < 64 and (np.diff(idx1) > 1).all()
    for c in C.CASES:
        idx0, idx1, _ = C.case_inputs(c)
        assert idx0.size == c.m and idx0.max() < c.n and idx1.max() < c.n


def test_the_fixture_is_this_tables():
    pinned = C.load_bits()                                        # asserts the keys and the shapes
    for c in C.CASES:
        p = pinned[c.key]
        if c.fails:
            assert p.code == -5 and "Cholesky pivot 0 <= 0 in Newton iteration 1" in p.message
            assert p.message.startswith("logit_posterior: " if c.entry == "binary" else "logit_posterior_multiclass: class 0: ")
            continue
        assert p.code == 0 and p.message == ""
        assert np.isfinite(p.mean.view(np.float64)).all() and np.isfinite(p.cov.view(np.float64)).all()
        assert c.m <= c.K or (p.cov.view(np.float64) >= c.sig[1]).all()      # the weight-space route: var >= sigma22 exactly
        assert (p.iters >= 1).all() and (p.iters <= c.max_iter).all()
        if c.max_iter == 2:
            assert (p.iters == 2).all()                           # the case is there for the cap
        if c.cols == C.MIXED_COLS and c.max_iter == 100:
            assert p.iters.min() == 2 < p.iters.max()
    with np.load(C.BITS_FILE) as z:
        assert len(str(z["commit"])) == 40 and str(z["hip"])
    assert os.path.getsize(C.BITS_FILE) < C.LARGEST_FIXTURE       # tests/golden/d16_r10.npz
