"""CPU: the case table of tests/regression_objective_cases.py covers what it says and tests/golden/regression_objective_bits.npz
is that table's.  The checked-in tests run against the committed fixture only; recording it is a manual step
(tests/golden/record_regression_objective_bits.py)."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regression_objective_cases as C  # noqa: E402

LARGEST_FIXTURE = 140707      # tests/golden/d16_r10.npz


def test_the_fixture_is_the_tables():
    with np.load(C.BITS_FILE) as z:
        assert [str(k) for k in z["keys"]] == [c.key for c in C.CASES + C.FAILURES]
        assert re.fullmatch(r"[0-9a-f]{40}", str(z["commit"]))
        n = len(z["keys"])
        assert z["value_bits"].shape == z["value_only_bits"].shape == z["code"].shape == z["message"].shape == (n,)
        off = z["grad_offsets"]
        assert off.shape == (n + 1,) and off[0] == 0 and off[-1] == z["grad_bits"].size
        for i, c in enumerate(C.CASES):
            assert off[i + 1] - off[i] == (c.m + 1 if c.noise == "different" else 2), c.key
            assert z["code"][i] == 0 and str(z["message"][i]) == ""
    assert os.path.getsize(C.BITS_FILE) < LARGEST_FIXTURE
    assert len(C.load_bits()) == len(C.CASES) + len(C.FAILURES)


def test_the_table_covers_every_route_noise_and_approach():
    assert len({c.key for c in C.CASES}) == len(C.CASES)
    for route, shapes in (("woodbury", C.WOODBURY), ("direct", C.DIRECT)):
        for noise in ("same", "different"):
            mine = [c for c in C.CASES if (c.route, c.noise) == (route, noise)]
            assert {c.q for c in mine} == {1, 3, 70} and {c.kind for c in mine} == {"range", "scattered"}
            assert {(c.K, c.m) for c in mine} == set(shapes)
            for approach in ("marginal", "posterior"):
                for K, m in shapes:
                    draws = [c for c in mine if (c.approach, c.K, c.m) == (approach, K, m)]
                    assert len(draws) == (1 if (noise, m) == ("different", 2500) else 2), (route, noise, approach, K, m)
                    assert len({c.pair for c in draws}) == len(draws)           # two x on two different pairs
                    assert len({C.inputs(c)[2].tobytes() for c in draws}) == len(draws)
    for c in C.CASES:
        assert (c.m > c.K) == (c.route == "woodbury") and (c.m <= c.K) == (c.route == "direct"), c.key
        assert c.K <= C.KP and 0 <= c.pair < len(C.PAIR_SEEDS)


def test_the_inputs_are_the_cases():
    for c in C.CASES:
        idx, Y, x = C.inputs(c)
        assert idx.shape == (c.m,) and Y.shape == (c.m, c.q) and x.shape == ((c.m + 1 if c.noise == "different" else 2),)
        if c.kind == "range":
            assert np.array_equal(idx, np.arange(100, 100 + c.m))
        assert 0 <= idx.min() and idx.max() < C.N and (x > 0).all()
