"""CPU: the shapes of tests/test_gpu_predictor_design_rows.py reach every path of the kernels of csrc/predictor_design.hip, by
the pure-Python model of tests/predictor_design_cases.py; and the constants of that model are the ones the source states."""
import os
import re

import predictor_design_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_constants_are_the_sources():
    src = open(os.path.join(ROOT, "flgp_amd", "csrc", "predictor_design.hip")).read()
    for name, value in (("PD_ROWS", dc.ROWS), ("PD_MAX_GRID", dc.MAX_GRID), ("PD_PICK_THREADS", dc.PICK), ("PD_LDS_S", dc.LDS_S)):
        m = re.search(r"constexpr int " + name + r" = (\d+);", src)
        assert m and int(m.group(1)) == value, name
    assert 8 * dc.LDS_S == 163840 and dc.ROWS % 64 == 0
    assert re.search(r"s <= 32768", src) and dc.SMAX == 32768
    hdr = open(os.path.join(ROOT, "include", "flgp_hip.h")).read()
    assert int(re.search(r"#define FLGP_RMAX (\d+)", hdr).group(1)) == dc.RMAX


def test_every_value_of_the_issue_is_in_the_table():
    ns, rs, ss, Ks, Bs = (sorted({c[i] for c in dc.CASES}) for i in range(5))
    assert set(ns) >= {1, 63, 64, 65, 257, 1000} and set(rs) == {1, 3, 10, 32} and set(Ks) >= {1, 15, 64, 65, 200}
    assert set(ss) >= {200, 20480, 20481} and any(s == r for _, r, s, _, _ in dc.CASES)
    assert all(K == 4 for _, _, s, K, _ in dc.CASES if s >= 20480)
    kinds = {("one" if B == 1 else "two" if B == 2 else "n" if B == n else "K+3" if B == K + 3 else "other") for n, r, s, K, B in dc.CASES}
    assert kinds >= {"one", "two", "n", "K+3"}
    assert all(dc.shape_ok(*c) for c in dc.CASES)


def test_the_table_reaches_every_path():
    w = [dc.walk(*c) for c in dc.CASES]
    assert any(x["p_in_lds"] for x in w) and any(not x["p_in_lds"] for x in w)
    assert {c[2] for c in dc.CASES if dc.walk(*c)["p_in_lds"]} >= {dc.LDS_S} and {c[2] for c in dc.CASES} >= {dc.LDS_S + 1}
    assert {c[1] for c in dc.CASES} >= {1, dc.RMAX}                                 # r from one entry to the ELL limit
    assert any(x["empty_lanes"] > 0 for x in w) and any(x["empty_lanes"] == 0 and x["lane_terms"] == 1 for x in w)    # K off and on 64
    assert any(x["uneven_lanes"] for x in w) and any(x["lane_terms"] == 4 for x in w)
    assert any(x["partials"] == 1 for x in w) and any(x["partials"] > 1 for x in w)
    assert any(x["ragged_wave"] for x in w) and any(not x["ragged_wave"] for x in w)
    assert any(x["last_range_rows"] == 1 for x in w)                                # a range of one row
    assert any(x["exhausted"] for x in w) and any(not x["exhausted"] for x in w)
    assert any(x["k_rounds"] == 2 for x in w) and any(x["tau_rounds"] == 2 for x in w)
    # at the knob 0 every workgroup walks one range; capped, some walk several, evenly and unevenly
    assert all(set(x["ranges_per_workgroup"]) == {1} for x in w)
    capped = [dc.walk(*c, knob=k) for c in dc.CASES for k in dc.caps(c[0])]
    assert any(max(x["ranges_per_workgroup"]) >= 4 and x["partials"] == 1 for x in capped)
    assert any(len(set(x["ranges_per_workgroup"])) == 2 and x["partials"] == 2 for x in capped)
    assert any(len(set(x["ranges_per_workgroup"])) == 1 and x["partials"] == 2 for x in capped)


def test_the_grid_and_the_workspace():
    assert dc.grid(1) == 1 and dc.grid(256) == 1 and dc.grid(257) == 2 and dc.grid(10 ** 6) == dc.MAX_GRID
    assert dc.grid(1000, 3) == 3 and dc.grid(1000, 0) == 4 and dc.grid(1000, 9) == 4
    # 12 n r for the rows, 9 n for the scores and marks, 16 K B for u: 12 + 0.9 + 3.2 MB at the timed 1e5 x 10, K = 200, B = 1000
    b = dc.workspace_bytes(100000, 10, 5000, 200, 1000)
    assert 12 * 10 ** 6 + 9 * 10 ** 5 + 16 * 200 * 1000 <= b <= 12 * 10 ** 6 + 9 * 10 ** 5 + 16 * 200 * 1000 + 8 * 5000 + 40000
