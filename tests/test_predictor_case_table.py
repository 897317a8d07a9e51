"""CPU: the case list of tests/test_gpu_predictor_rows.py reaches every way predictor_rows_kernel walks a shape, by the
pure-Python model of tests/predictor_cases.py."""
import predictor_cases as pc


def test_the_column_shapes_reach_every_chunk_count_tail_and_mean_place():
    walks = [pc.walk(K, q) for K, q in pc.KQ]
    assert {w["chunks"] for w in walks} == {1, 2, 3, 4}
    assert {w["place"] for w in walks} == {"none", "behind the squares", "own chunk", "straddles"}
    assert 64 in {w["tail"] for w in walks} and {w["tail"] for w in walks} & set(range(1, 64))        # full and partial last chunks
    assert {w["square_terms_per_lane"] for w in walks} >= {1, 2, 4}
    assert pc.walk(63, 1)["tail"] == 64 and pc.walk(62, 1)["tail"] == 63 and pc.walk(64, 1)["tail"] == 1
    # skipping an output changes the range: the mean alone starts at the chunk of column K, the variance alone ends with K
    mean_only = [pc.walk(K, q, var=False) for K, q in pc.KQ if q]
    assert {w["c_lo"] for w in mean_only} >= {0, 1, 3} and all(w["chunks"] >= 1 for w in mean_only)
    assert pc.walk(127, 2, var=False) == dict(c_lo=1, chunks=2, tail=1, place="straddles", square_terms_per_lane=0)
    var_only = [pc.walk(K, q, mean=False) for K, q in pc.KQ]
    assert {w["chunks"] for w in var_only} == {1, 2, 4} and all(w["place"] == "none" for w in var_only)
    assert pc.walk(64, 1, mean=False)["chunks"] == 1 and pc.walk(64, 1)["chunks"] == 2


def test_the_row_counts_reach_every_workgroup_edge():
    grids = [pc.grid(n, g) for n in pc.NS for g in pc.GROUPS]
    assert {g["blocks"] for g in grids} >= {1, 16, 17, 65}
    assert {g["last_block_rows"] for g in grids} == {1, 3, 4}            # a lone row, a partial and a full last workgroup
    assert {g["grid_y"] for g in grids} == {1, 3}
    assert min(pc.RS) == 1 and max(pc.RS) == pc.RMAX and pc.S >= pc.RMAX
