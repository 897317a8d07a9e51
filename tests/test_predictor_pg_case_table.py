"""CPU: the case list of tests/test_gpu_predictor_pg_rows.py reaches every way predictor_pg_rows_kernel walks a shape, by the
pure-Python model of tests/predictor_pg_cases.py; and the numpy restatement (tests/np_predictor_pg.py) has the properties the
GPU tests lean on: first arg-max at ties, saturation without NaN."""
import numpy as np

import np_predictor_pg as npg
import predictor_pg_cases as pc


def test_the_chain_counts_reach_every_chunk_count_tail_and_lane_load():
    walks = {B: pc.walk(B) for B in pc.BS}
    assert {w["chunks"] for w in walks.values()} == {1, 2, 3}
    assert {w["tail"] for w in walks.values()} >= {1, 2, 63, 64}                # a lone lane, a partial and a full last chunk
    assert walks[64]["idle_lanes"] == 0 and walks[63]["idle_lanes"] == 1 and walks[1]["idle_lanes"] == 63
    assert walks[65] == dict(chunks=2, tail=1, idle_lanes=0, one_chain_lanes=63, many_chain_lanes=1, link=True, butterfly=True)
    assert walks[130]["many_chain_lanes"] == 64 and walks[130]["tail"] == 2    # lanes 0, 1 hold three chains, the others two
    assert all(w["idle_lanes"] + w["one_chain_lanes"] + w["many_chain_lanes"] == 64 for w in walks.values())


def test_the_output_subsets_reach_both_sides_of_the_link_and_the_butterfly():
    assert len(pc.SUBSETS) == 15 and len(set(pc.SUBSETS)) == 15
    seen = {(pc.walk(65, o)["link"], pc.walk(65, o)["butterfly"]) for o in pc.SUBSETS}
    assert seen == {(False, False), (True, False), (True, True)}               # f alone; a link without a label; a label
    assert [o for o in pc.SUBSETS if not pc.walk(1, o)["link"]] == [("f",)]


def test_the_row_counts_reach_every_workgroup_edge():
    grids = [pc.grid(n) for n in pc.NS]
    assert {g["blocks"] for g in grids} == {1, 2, 65}
    assert {g["last_block_rows"] for g in grids} == {1, 3, 4}                  # a lone row, a partial and a full workgroup
    assert min(pc.RS) == 1 and max(pc.RS) == pc.RMAX
    assert min(pc.SS) == 1 and max(pc.SS) > pc.RMAX
    assert len(pc.shapes(1)) == len(pc.RS) * len(pc.SS)


def test_the_restatement_takes_the_first_maximum_and_saturates_cleanly():
    idx = np.array([[0, 2], [1, 1]]); val = np.array([[1.0, 2.0], [0.5, 0.25]])
    P = np.array([[1.0, -1.0], [4.0, 8.0], [0.5, 3.0]])
    f = npg.latent(idx, val, P, 2)
    np.testing.assert_array_equal(f, [[(0.0 + 1.0 * 1.0) + 2.0 * 0.5, (0.0 - 1.0) + 6.0], [(0.0 + 2.0) + 1.0, (0.0 + 4.0) + 2.0]])
    pi, y, label = npg.link(np.array([[0.0, 0.0, -1.0], [40.0, 50.0, 60.0], [-800.0, -800.0, -800.0], [1.0, 3.0, 3.0]]))
    np.testing.assert_array_equal(label, [0.0, 0.0, 0.0, 1.0])                # ties (0.5; 1.0 exactly; 0.0): the lowest index
    assert pi[1].tolist() == [1.0, 1.0, 1.0] and pi[2].tolist() == [0.0, 0.0, 0.0] and not np.isnan(pi).any()
    np.testing.assert_array_equal(y, [[0, 0, 0], [1, 1, 1], [0, 0, 0], [1, 1, 1]])


def test_the_chain_restatement_is_the_collapsed_prediction():
    """V2 u is Cnv w: the latent the batch entry forms for a row of the pair"""
    import np_pg
    rng = np.random.default_rng(3)
    m, K, t, sigma = 9, 4, 1.5, 1e-2
    V = rng.normal(size=(m + 5, K)); values = np.sort(rng.uniform(0.2, 1.0, K))[::-1]
    Y = (rng.uniform(size=m) < 0.5).astype(float); omega = rng.uniform(0.1, 0.3, m)
    u = npg.chain_u(V[:m], values, K, t, sigma, omega, Y)
    l, _ = np_pg.weights(values, K, t)
    C = V[:m] @ (l[:, None] * V[:m].T) + sigma * np.eye(m)
    w = np_pg.collapsed_w(omega, Y - 0.5, C)
    np.testing.assert_allclose(V[m:] @ u, (V[m:] @ (l[:, None] * V[:m].T)) @ w, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(npg.fold(V[m:], u[:, None])[:, 0], V[m:] @ u, rtol=0, atol=0)
