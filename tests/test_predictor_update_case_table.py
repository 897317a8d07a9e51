"""CPU: the shapes of tests/test_gpu_predictor_gram.py reach every edge of the kernels of csrc/predictor_update.hip, by the
pure-Python model of tests/predictor_update_cases.py; and the constants of that model are the ones the source states."""
import os
import re

import predictor_update_cases as uc
import np_predictor_update as npu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_constants_are_the_sources():
    src = open(os.path.join(ROOT, "flgp_amd", "csrc", "predictor_update.hip")).read()
    m = re.search(r"constexpr int PG_CT = (\d+), PG_STEP = (\d+), PG_GC = (\d+), PG_WAVES = (\d+), PG_LD = (\d+);", src)
    assert m, "the constants line of predictor_update.hip"
    ct, step, gc, waves, ld = map(int, m.groups())
    assert (ct, step, gc, waves) == (uc.CT, uc.STEP, uc.GC, uc.WAVES) == (npu.CT, npu.STEP, npu.GC, uc.WAVES)
    assert gc % step == 0 and step % (4 * waves) == 0 and ct == 16 * waves          # whole steps, whole k-steps per wave, a block row per wave
    assert ld >= ct and ld % 32 == 16                                               # two rows of a half wave on disjoint bank halves
    assert 2 * step * ld * 8 <= 64 * 1024                                           # the two tiles in static LDS


def test_rows_reach_every_edge():
    w = [uc.walk(n, 14, 1) for n in uc.NS]
    assert [x["chunks"] for x in w] == [1, 1, 1, 1, 1, 1, 2, 3]
    assert {x["last_step_rows"] for x in w} >= {1, uc.STEP - 1, uc.STEP, 3}
    assert any(x["idle_waves"] == 3 for x in w) and any(x["idle_waves"] == 0 and x["partial_step"] for x in w)
    assert any(x["ragged_k_step"] for x in w) and any(not x["partial_step"] for x in w)
    assert any(x["steps_in_last_chunk"] == uc.GC // uc.STEP for x in w)             # a whole chunk
    assert any(x["chunks"] == 2 and x["last_chunk_rows"] == 1 for x in w)           # a chunk of one row
    assert max(uc.NS) <= 2 ** 14                                                    # the exact test's sums stay below 2^53


def test_columns_reach_every_edge():
    w = {kq: uc.walk(1, *kq) for kq in uc.KQS}
    W = sorted({k + q for k, q in uc.KQS})
    for edge in (uc.BLK, uc.CT):
        assert {edge - 1, edge, edge + 1} <= set(W), edge
    assert {q for _, q in uc.KQS} == {1, 3}
    assert {x["tiles"] for x in w.values()} >= {1, 2, 3, 4} and {x["panels"] for x in w.values()} >= {1, 3, 6, 10}
    assert any(x["mean_straddles_a_tile"] for x in w.values())                      # the residual is taken in two tiles
    assert any(x["tiles"] == 2 and x["last_tile_cols"] == 1 for x in w.values())    # a tile of one column
    assert any(x["partial_block"] for x in w.values()) and any(not x["partial_block"] for x in w.values())
    assert any(x["empty_blocks_in_last_tile"] == 3 for x in w.values())
    assert any(x["mean_tile"] >= 1 for x in w.values()) and any(x["mean_tile"] == 0 for x in w.values())
    assert uc.RS == [1, 5, 32] and uc.SS == [1, 7, 300] and uc.LDP_PAD > 0 and uc.LDS_PAD > 0


def test_the_panels_cover_the_lower_triangle_once():
    for T in (1, 2, 3, 4, 32):
        seen = [uc.panel_of(p) for p in range(T * (T + 1) // 2)]
        assert sorted(seen) == [(i, j) for i in range(T) for j in range(i + 1)]
    for I, J in ((0, 0), (2, 2)):
        assert [len(uc.blocks_of(I, J, w)) for w in range(uc.WAVES)] == [1, 2, 3, 4]
    assert [len(uc.blocks_of(2, 1, w)) for w in range(uc.WAVES)] == [4, 4, 4, 4]


def test_the_order_cases_cover_one_and_several_chunks():
    chunks = [uc.walk(n, K, q)["chunks"] for _, _, K, q, n in uc.ORDER_CASES]
    assert 1 in chunks and 2 in chunks and 3 in chunks
    assert any(uc.walk(n, K, q)["panels"] > 1 for _, _, K, q, n in uc.ORDER_CASES)


def test_the_update_block_is_a_multiple_of_the_chunk():
    for blk in (1, 256, 1000, 1024, 5000, 1 << 20):
        b = uc.update_block(blk)
        assert b % uc.GC == 0 and b >= uc.GC and b <= max(blk, uc.GC)
    assert uc.update_block(256) == uc.GC and uc.update_block(1 << 20) == 1 << 20


def test_the_launches_and_the_workspace():
    assert uc.launch_chunks(200, 1) == 64 and uc.launch_chunks(2000, 1) == 8 and uc.launch_chunks(20000, 1) == 1
    assert uc.launches(64 * uc.GC, 200, 1) == 1 and uc.launches(64 * uc.GC + 1, 200, 1) == 2
    n = max(uc.NS)                                                                  # three chunks: 3, 2 and 1 launches
    assert [uc.launches(n, 14, 3, knob) for knob in (1, 2, 64)] == [3, 2, 1]
    assert uc.workspace_bytes(100000, 200, 1) == 64 * 8 * 201 ** 2                  # 20.7 MB whatever n is
    assert uc.workspace_bytes(n, 14, 3, 1) == 8 * 17 ** 2
