"""CPU: the case tables of test_gpu_hk_edges.py reach every edge of hk_panel2_kernel (csrc/hk2.hip) and hk_panel_kernel
(csrc/hk.hip) they are there for -- shown with the restatement in hk_cases.py, so that a table that drifts fails here
instead of silently testing less -- and the library's own workspace query covers the scaled small operand in both layouts
for every K (flgp_dev_hk_workspace is host arithmetic: no GPU)."""
import hk_cases as C
from flgp_amd import _lib

PANEL_GRID_PAIRS = {(1, 1), (2, 1), (3, 1), (5, 2), (7, 3)}
REMAINDERS = {0, 1, 17, 63}


def tuned_route(cs):
    return C.route(cs["n0"], cs["n1"], cs["K"], cs["n0"] + 5, C.case_tuning(cs))


def panel_requirements(facts):
    """what both tables must reach in the loop over panels"""
    assert {(f["panels"], f["grid"]) for f in facts} >= PANEL_GRID_PAIRS
    assert {f["rem"] for f in facts if f["panels"] > 1} >= REMAINDERS
    assert any(f["panels"] == 1 and 0 < f["rem"] for f in facts), "n0 < 64"
    assert any(f["uneven"] for f in facts), "an uneven number of panels per workgroup"
    assert any(f["ragged_by_prefetch"] for f in facts), "a ragged last panel that arrives through the prefetch"
    assert any(f["ragged_by_prefetch"] and f["grid"] > 1 for f in facts)
    assert any(f["refetch_other"] for f in facts), "next panel clamped to the last one, which is another workgroup's"


def test_restated_dispatch():
    assert [C.nks(K) for K in (88, 89, 104, 105, 112, 113, 184, 185, 208, 209)] == [0, 26, 26, 28, 28, 0, 0, 52, 52, 0]
    assert (C.na(26), C.na(28), C.na(52)) == (26, 28, 26)
    for n in (26, 28, 52):
        assert (2 * C.na(n) + n - C.na(n)) * 2048 <= C.LDS_MI355X
    # with nothing tuned: the path's shapes, and the thresholds
    assert C.route(100000, 1000, 200, 100000) == 2 and C.route(100000, 479, 200, 100000) == 1
    assert C.route(100000, 1000, 120, 100000) == 1 and C.route(100000, 63, 120, 100000) == 0
    assert C.route(2047, 1000, 200, 2047) == 0 and C.route(100000, 1000, 289, 100000) == 0
    assert C.route(100000, 1000, 200, 100000, {"hk_panel2": 0}) == 1 and C.route(100000, 1000, 200, 100000, {"hk_panel": 0}) == 0
    # the K at which hk.hip's buffer is the smaller one are exactly these
    short = [K for K in range(1, 301) if 4 * C.nks(K) > C.ceil16(K)]
    assert short == list(range(89, 97)) + list(range(185, 193))


def test_hk2_table_reaches_every_edge():
    cases = C.HK2_CASES
    assert all(c["n0"] <= 7 * 64 and c["n1"] <= 545 and c["K"] <= 288 for c in cases)
    assert all(tuned_route(c) == 2 for c in cases)
    facts = [C.hk2_facts(c["n0"], c["n1"], c["K"], c["grid"]) for c in cases]
    panel_requirements(facts)
    Ks = {c["K"] for c in cases}
    assert {f["nks"] for f in facts} == {26, 28, 52}
    assert Ks >= {89, 104, 105, 112, 185, 208}
    assert Ks & set(range(90, 97)) and Ks & set(range(186, 193)), "one K inside each range where hk2's layout is the larger"
    assert {K % 4 for K in Ks} == {0, 1, 2, 3}
    assert any(f["a_copies_reused"] for f in facts), "both A copies written a second time"
    assert {c["n1"] for c in cases} >= {20, 33, 256, 257, 520, 545}
    by_n1 = {c["n1"]: f for c, f in zip(cases, facts)}
    assert by_n1[20]["npairs"] == 1 and by_n1[20]["idle_waves"] == 7
    assert by_n1[33]["tile_outside_n1"]
    assert by_n1[256]["ntw"] == [1] * 8 and by_n1[257]["ntw"] == [2] + [1] * 7
    assert set(by_n1[520]["ntw"]) == {2, 3} and set(by_n1[545]["ntw"]) == {2, 3}
    # a wave without tiles carries its share of the next panel, in every instance (the 52-step one also its B part)
    assert {f["nks"] for f in facts if f["idle_wave_carries_next"]} == {26, 28, 52}
    # NKS = 26: thirteen ring stages, the parity alternates -- P1 as a non-last and as a last tile, P0 as both too
    t26 = set().union(*(f["tiles"] for f in facts if f["nks"] == 26))
    assert t26 == {(False, 0), (False, 1), (True, 0), (True, 1)}
    for n in (28, 52):
        assert set().union(*(f["tiles"] for f in facts if f["nks"] == n)) == {(False, 0), (True, 0)}
    # the 52-step instance keeps a B part: more than one panel per workgroup with it
    assert any(f["nks"] == 52 and f["nb"] == 26 and max(f["per_wg"]) >= 3 for f in facts)
    assert {c["idx1"] for c in cases} == {"range", "repeat"} and any(c["gather0"] for c in cases)
    for lo, hi in ((89, 96), (185, 192)):
        assert any(lo <= c["K"] <= hi and c["gather0"] for c in cases), "gathered idx0 where the overrun reached the gathered rows"


def test_hk_table_reaches_every_edge():
    cases = C.HK_CASES
    assert all(c["n0"] <= 7 * 64 and c["n1"] <= 545 and c["K"] <= 288 for c in cases)
    assert all(tuned_route(c) == 1 for c in cases)
    facts = [C.hk_facts(c["n0"], c["n1"], c["K"], c["grid"]) for c in cases]
    panel_requirements(facts)
    assert {f["PG"] for f in facts} == {7, 9}
    assert any(f["PG"] == 9 and f["has_next"] for f in facts), "the PG = 9 instance with a next panel"
    assert {f["nst"] for f in facts} >= {1, 14, 15, 18}
    assert any(c["K"] % 16 and c["K"] % 4 for c in cases) and any(c["K"] % 16 == 0 for c in cases)
    assert {c["n1"] for c in cases} >= {1, 16, 17, 128, 129, 130}
    for n1 in (1, 16):
        assert any(c["n1"] == n1 and f["f0_with_next"] for c, f in zip(cases, facts)), "waves with F = 0 while has_next"
    assert any(f["f0_with_next"] and f["PG"] == 7 for f in facts) and any(f["f0_with_next"] and f["PG"] == 9 for f in facts)
    assert any(c["n1"] == 128 and set(f["pf_at"]) == {0} and f["has_next"] for c, f in zip(cases, facts)), "pf_at == 0"
    assert any(max(f["pf_at"]) > 0 and f["has_next"] for f in facts)
    for n1 in (129, 130):
        assert any(c["n1"] == n1 and f["rollover_mid_turn"] for c, f in zip(cases, facts))
    assert any(f["rollover_in_ring"] and not f["rollover_mid_turn"] for f in facts)
    assert set().union(*(f["fmod4_with_next"] for f in facts)) == {0, 1, 2, 3}
    assert {c["idx1"] for c in cases} == {"range", "repeat"} and {c["gather0"] for c in cases} == {False, True}


def test_route_boundary_table():
    assert tuple(c["K"] for c in C.ROUTE_CASES) == (88, 113, 184, 209, 288, 289)
    assert [tuned_route(c) for c in C.ROUTE_CASES] == [1, 1, 1, 1, 1, 0]
    for K in (89, 112, 185, 208):
        assert C.route(129, 33, K, 134, C.case_tuning(C.ROUTE_CASES[0])) == 2
    for cs, kernel in ((C.ROUNDING_HK2, 2), (C.ROUNDING_HK, 1)):
        assert tuned_route(cs) == kernel and C.panel_facts(cs["n0"], cs["grid"])["panels"] > cs["grid"]


def test_workspace_covers_both_layouts_for_every_K():
    """flgp_dev_hk_workspace(n0, n1, K, 0) holds the scaled small operand as either panel kernel lays it out: n1 padded to 32
    rows x max(K padded to 16, 4 nks(K)) columns.  (Sized by the first alone it was 8 or 16 columns short for K in 89..96
    and 185..192: hk2_scale_kernel wrote past it, into the gathered rows of V0 where there were any.)"""
    L = _lib.lib()
    short = []
    for K in range(1, 301):
        for n1 in (1, 31, 32, 33, 480, 1000):
            for n0 in (1, 2100):
                if L.flgp_dev_hk_workspace(n0, n1, K, 0) < 8 * C.vw_elems(n1, K):
                    short.append((n0, n1, K))
            # the gathered rows of V0 lie behind it
            assert L.flgp_dev_hk_workspace(2100, n1, K, 1) >= L.flgp_dev_hk_workspace(2100, n1, K, 0) + 8 * 2100 * K
    assert not short, "workspace smaller than the operand hk2_scale_kernel writes, K = %s" % sorted({k for _, _, k in short})
