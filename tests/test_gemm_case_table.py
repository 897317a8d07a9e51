"""CPU: the case tables of test_gpu_gemm_edges.py reach every path of csrc/gemm.hip's dispatch.

plan() (gemm_cases.py) restates the dispatch in Python; features() names the paths a planned call takes.  The tables must
reach every combination that exists, per tile size, so an edit of the tables cannot drop a path without this file noticing.
(That plan() itself tells the truth is checked on the GPU: the planes it predicts against the launch's own count.)"""
import itertools

import pytest

import gemm_cases as G


def feats(cases):
    got = set()
    for cs in cases:
        got |= G.features(G.case_plan(cs))
    return got


def test_tables_reach_every_path():
    missing = G.required_features() - feats(G.all_plain_cases())
    assert not missing, sorted(missing, key=str)


@pytest.mark.parametrize("tile", [64, 128])
def test_stage_ring_table(tile):
    """the four fast staging pairs and a GEN operand, each over the whole list of depths; in the 64-tile the FAST and the
    plain pipeline each with ns mod 3 in {0, 1, 2}, and 0, 1, 2 stages"""
    for modes in G.RING_MODES:
        cases = G.stage_ring_cases(tile, modes)
        assert [cs["Kd"] for cs in cases] == list(G.RING_KD)
        ma, mb = modes.split("-")
        for cs in cases:
            p = G.case_plan(cs)
            assert p["tile"] == tile and not p["swap"] and p["planes"] == 1 and len(p["tiles"]) == 1
            assert (p["tiles"][0]["a"], p["tiles"][0]["b"]) == (ma, mb), G.case_id(cs)
            assert p["tiles"][0]["fast"][0] == (tile == 64 and ma != "GEN" and cs["Kd"] % 2 == 0 and cs["Kd"] > 0), G.case_id(cs)
        got = feats(cases)
        assert {(tile, "ns", n) for n in (0, 1, 2)} <= got
        if tile == 64:
            kinds = ("plain",) if ma == "GEN" else ("fast", "plain")
            assert {(64, k, "ns%3", m) for k in kinds for m in (0, 1, 2)} <= got, modes


@pytest.mark.parametrize("tile", [64, 128])
def test_tile_table_is_pairwise_complete(tile):
    """every M against every N; per operand every (layout, pad, offset); per pair of operands every pair of (pad, offset);
    all eight layouts; every epilogue on both layouts of C"""
    cases = [cs for M in G.TILE_MN for cs in G.tile_cases(tile, M)]
    assert {(cs["M"], cs["N"]) for cs in cases} == set(itertools.product(G.TILE_MN, repeat=2))
    every = set(itertools.product(("row", "k"), G.PADS, G.OFFSETS))
    for op in "abc":
        assert {cs[op] for cs in cases} == every, op
    for x, y in ("ab", "ac", "bc"):
        assert {(cs[x][1:], cs[y][1:]) for cs in cases} == set(itertools.product(G.PADOFF, repeat=2)), x + y
    assert {(cs["a"][0], cs["b"][0], cs["c"][0]) for cs in cases} == set(G.LAYOUTS8)
    assert {(cs["e"], cs["e2"], cs["c"][0]) for cs in cases} == {(e, e2, c) for e, e2 in G.EPI4 for c in ("row", "k")}
    got = feats(cases + G.tile_extra_cases(tile))
    need = {f for f in G.required_features() if f[0] == tile and f[1] in ("modes", "gen", "shifted")}
    need |= {(tile, "not shifted", "smaller than a tile")}
    need |= {(tile, "epilogue", e, w) for e in ("none", "E", "E2", "E+E2") for w in ("inside", "edge")}
    assert need <= got, sorted(need - got, key=str)


@pytest.mark.parametrize("tile", [64, 128])
def test_heat_kernel_shape_is_in_the_table(tile):
    """an odd row count on an even leading dimension from an aligned base: RC staging from an odd shifted row0"""
    cs = G.tile_extra_cases(tile)[0]
    p = G.case_plan(cs)
    a_is, a_ks = G.case_strides(cs)[:2]
    assert cs["M"] % 2 == 1 and a_is == 1 and a_ks % 2 == 0 and cs["a"][2] == 0 and p["tile"] == tile
    rows = [t for t in p["tiles"] if (t["shift_col"] if p["swap"] else t["shift_row"])]
    assert rows and all((t["b"] if p["swap"] else t["a"]) == "RC" and (t["col0"] if p["swap"] else t["row0"]) % 2 == 1 for t in rows)


def test_default_dispatch_takes_the_128_tile():
    one, two = (G.case_plan(cs) for cs in G.default128_cases())
    assert one["tile"] == 128 and one["planes"] == 1
    assert two["tile"] == 128 and two["planes"] == 2


@pytest.mark.parametrize("tile", [64, 128])
def test_in_place_cases_cover_both_edge_policies(tile):
    cases = [cs for cs in G.epilogue_cases(tile) if "C" in (cs["e"], cs["e2"])]
    plans = [G.case_plan(cs) for cs in cases]
    assert all(min(cs["M"], cs["N"]) >= tile and (cs["M"] % tile or cs["N"] % tile) for cs in cases)
    assert any(not p["shift_edges"] and p["planes"] == 1 for p in plans)       # aliased, not split: no overlapping tiles
    assert any(p["shift_edges"] and p["planes"] > 1 for p in plans)            # split: the reduction writes every element once
    assert all(p["aliased"] for p in plans)


@pytest.mark.parametrize("tile", [64, 128])
def test_split_table(tile):
    cases = G.splitk_cases(tile)
    assert {cs["Kd"] for cs in cases} == set(G.SPLIT_KD) and {cs["force_split"] for cs in cases} == set(G.FORCE)
    assert {(64, 64), (130, 70)} <= {(cs["M"], cs["N"]) for cs in cases}
    got = feats(cases)
    assert {(tile, "planes", 1), (tile, "planes", 2), (tile, "planes", 3), (tile, "ragged last plane"),
            (tile, "epilogue", "planes", "inside"), (tile, "epilogue", "planes", "edge")} <= got
    for cs in cases:                       # a forced count is taken as given, up to the rounding of klen to whole stages
        p = G.case_plan(cs)
        assert not p["invalid"]
        if cs["force_split"]:
            assert p["planes"] <= cs["force_split"]


def test_plan_restates_the_documented_examples():
    """figures the library's own comments and callers state"""
    # the eigensolver's 256 x 256 x 5000 Gram product: 16 tiles of 64 -> 16 planes of 320 (rot.hip's ranges coincide with them)
    p = G.plan(256, 256, 5000, 5000, 1, 1, 5000, 1, 256, work_elems=64 * 256 * 256)
    assert (p["tile"], p["planes"], p["klen"]) == (64, 16, 320) and p["swap"]
    # no workspace: never split
    assert G.plan(64, 64, 5000, 1, 64, 1, 5000, 1, 64)["planes"] == 1
    # a forced split without the room for it is refused
    assert G.plan(64, 64, 5000, 1, 64, 1, 5000, 1, 64, work_elems=64 * 64, force_split=2)["invalid"]
    # Kd = 0: one plane, no stages
    p = G.plan(64, 64, 0, 1, 64, 1, 0, 64, 1)
    assert p["planes"] == 1 and p["z"][0]["ns"] == 0
