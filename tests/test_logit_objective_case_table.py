"""CPU: the pinned cases of the logit objective (logit_objective_cases.GROUPS) cover what they are meant to, and the
device-recorded fixture tests/golden/logit_objective_bits.npz is the one of this table."""
import numpy as np

import logit_objective_cases as C


def test_the_table_covers_every_shape_kind_sigma_and_configuration():
    keys = [g.key for g in C.GROUPS]
    assert len(set(keys)) == len(keys)
    low = [g for g in C.GROUPS if g.m > g.K and g.max_iter == 100]
    assert {(g.K, g.m, g.kind, g.sigma, g.config) for g in low} == {
        (K, m, kind, sigma, config) for K, m in C.LOWRANK_SHAPES for kind in ("perm", "repeated") for sigma in (1e-3, 0.1)
        for config in ("indicator", "binomial")}
    dense = [g for g in C.GROUPS if g.m <= g.K]
    assert {(g.K, g.m, g.config) for g in dense} == {(K, m, c) for K, m in C.DENSE_SHAPES for c in ("indicator", "binomial")}
    assert sorted((g.K, g.m) for g in C.GROUPS if g.max_iter == 2) == sorted(C.LOWRANK_SHAPES)
    for g in C.GROUPS:
        cols, ts = C.problems(g)
        assert set(zip(cols.tolist(), ts.tolist())) == {(c, t) for c in range(5 if g.config == "indicator" else 6) for t in C.TS}


def test_the_fixture_is_this_tables():
    pinned = C.load_bits()                                        # asserts the keys, columns and values of t
    for g in C.GROUPS:
        bits, iters = pinned[g.key]
        assert bits.dtype == np.uint64 and iters.dtype == np.int32
        assert np.isfinite(bits.view(np.float64)).all() and (iters >= 1).all() and (iters <= g.max_iter).all()
        if g.max_iter == 2:
            assert (iters == 2).all()                             # the case is there for the cap
    with np.load(C.BITS_FILE) as z:
        assert len(str(z["commit"])) == 40 and str(z["hip"])
