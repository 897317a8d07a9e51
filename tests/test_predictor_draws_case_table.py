"""CPU: the shapes of the f-23 GPU tests reach every edge of the kernels they run (tests/predictor_draws_cases.py models the
walk), and the restatements of tests/np_predictor_draws.py say what the header says: the cols chain is np_predictor.rows's
chain, the fold is mean + Z xi reassociated, the streams are (g q + c) 2^32 + t of flgp_amd/synth.py."""
import itertools
import os
import re

import numpy as np

import np_predictor as npp
import np_predictor_draws as npd
import predictor_draws_cases as pc
from flgp_amd import synth


def test_cols_shapes_reach_every_tile_edge():
    walks = [pc.tiles(n, nc, c0) for n, nc, c0 in itertools.product(pc.NS, pc.NCS, pc.C0S)]
    kinds = {(w["partial_rows"], w["partial_cols"]) for w in walks}
    assert kinds == {(False, False), (False, True), (True, False), (True, True)}
    # a first tile that is also the last and partial, and a last tile behind full ones, in rows, in columns and in both
    for single in (True, False):
        assert any(w["first_tile_is_last"][0] == single and w["partial_rows"] for w in walks)
        assert any(w["first_tile_is_last"][1] == single and w["partial_cols"] for w in walks)
        assert any(w["first_tile_is_last"] == (single, single) and w["partial_rows"] and w["partial_cols"] for w in walks)
    assert {w["idle_waves"] for w in walks} >= {0, 3}                      # a tile of one row leaves three waves without work
    assert {w["aligned"] for w in walks} == {True, False}                  # c0 = 3 is no multiple of 64
    assert {w["row_tiles"] for w in walks} >= {1, 2, 5} and {w["col_tiles"] for w in walks} >= {1, 2, 3}
    assert min(pc.RS) == 1 and max(pc.RS) == 32                            # the ends of the broadcast
    assert any(r > s for r in pc.RS for s in pc.SS)                        # indices repeat within a row


def test_routing_of_the_cols_entry():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flgp_amd", "csrc", "predictor_cols.hip")).read()
    assert re.search(r"PC_TILE_MIN = %d;" % pc.TILE_MIN, src) and re.search(r'tuning\("predictor_cols_tile_min", PC_TILE_MIN\)', src)
    assert {pc.cols_route(nc) for nc in pc.NCS} == {"pg_rows"}                # at the default the kernel tests would miss the tile kernel
    assert {pc.cols_route(nc, 1) for nc in pc.NCS} == {"tile"}                # so they set the knob to 1
    assert [pc.cols_route(nc) for nc in pc.ROUTED_NCS] == ["pg_rows", "tile", "tile"]
    assert pc.tiles(65, 577)["partial_cols"] and not pc.tiles(65, 512)["partial_cols"]


def test_fold_shapes_reach_every_chunk_edge():
    walks = [pc.fold_walk(s, K, g, q, S) for s, K, (g, q), S in itertools.product(pc.FOLD_S, pc.FOLD_K, pc.FOLD_GQ, pc.FOLD_DRAWS)]
    walks += [pc.fold_walk(s, K, g, q, S) for s, K, (g, q), S in pc.FOLD_EXTRA]
    assert {w["col_blocks"] for w in walks} == {1, 2} and any(w["col_blocks"] == 2 and w["last_block_cols"] == 44 for w in walks)
    assert {w["last_pass_rows"] for w in walks} >= {1, 7, 4}               # 300 = 37 * 8 + 4: a partial pass behind full ones
    assert {w["passes"] for w in walks} >= {1, 38}
    assert {w["planes"] for w in walks} == {1, 3}
    assert {w["last_block_cols"] for w in walks} >= {1, 5, 64, 65, 192, 195}
    assert {w["waves_in_last_block"] for w in walks} >= {1, 2, 4}          # a wave that is partly on, and whole waves off
    assert {w["chain"] for w in walks} >= {1, 63, 64, 65, 130}             # K on both sides of 64
    ncols = {w["ncol"] for w in walks}
    assert min(ncols) == 1 and any(n <= 8 for n in ncols) and any(8 < n <= 64 for n in ncols) and any(n > 64 for n in ncols)


def test_handle_shapes_reach_both_nystrom_routes_and_both_sides_of_64():
    ncols = [g * q * S for g, q, S in pc.HANDLE_DRAWS]
    assert {pc.nystrom_route("draws", n) for n in ncols} == {"mean", "cols"}
    assert pc.nystrom_route("draws", 8) == "mean" and pc.nystrom_route("draws", 9) == "cols"
    assert pc.nystrom_route("regression", 3) == "cols"                      # features never take the mean route
    assert any(n <= 8 for n in ncols) and any(8 < n <= 64 for n in ncols) and any(n > 64 for n in ncols)
    assert any(K < 64 for K in pc.HANDLE_K) and any(K > 64 for K in pc.HANDLE_K)
    assert {pc.tiles(pc.BIT_ROWS, n)["partial_cols"] for n in ncols} == {True}
    assert pc.tiles(pc.BIT_ROWS, 130)["col_tiles"] == 3 and pc.tiles(pc.BIT_ROWS, 200)["col_tiles"] == 4
    assert pc.BIT_ROWS % 256 == 1 and pc.BIT_ROWS % pc.PC_TILE == 1        # a block and a tile of one row


def _problem(seed, n=37, r=5, s=23, groups=2, K=9, q=2):
    rng = np.random.default_rng(seed)
    idx = np.sort(np.stack([rng.permutation(s)[:r] for _ in range(n)]), axis=1)
    val = rng.normal(size=(n, r))
    P = rng.normal(size=(s, groups * (K + q) + 3))
    return idx, val, P, groups, K, q


def test_cols_is_the_chain_of_the_row_kernel():
    idx, val, P, groups, K, q = _problem(1)
    w = K + q
    mean, var = npp.rows(idx, val, P, groups, K, q, np.zeros(groups))
    for g in range(groups):
        np.testing.assert_array_equal(npd.cols(idx, val, P, g * w + K, q), mean[:, g * q:(g + 1) * q])
        Z = npd.cols(idx, val, P, g * w, K)
        assert np.abs(var[:, g] - (Z * Z).sum(1)).max() <= (K + 8) * 2.0 ** -53 * (Z * Z).sum(1).max()
    np.testing.assert_array_equal(npd.cols(idx, val, P, 3, 7), npd.cols(idx, val, P, 0, 12)[:, 3:10])     # a column is its own chain


def test_streams_and_normals():
    seed, K, groups, q, S = 12345, 6, 2, 3, 4
    xi = npd.normals(seed, K, groups, q, S)
    for g, c, t in itertools.product(range(groups), range(q), range(S)):
        assert npd.stream_of(g, c, t, q) == (g * q + c) * 2 ** 32 + t
        np.testing.assert_array_equal(xi[:, (g * q + c) * S + t], synth.normal(seed, npd.stream_of(g, c, t, q), K))
    # a draw does not depend on S, and a longer chain starts with the shorter one
    big = npd.normals(seed, K + 5, groups, q, S + 3)
    for gc, t in itertools.product(range(groups * q), range(S)):
        np.testing.assert_array_equal(big[:K, gc * (S + 3) + t], xi[:, gc * S + t])
    rad = npd.radius(seed, K, groups, q, S)
    assert (np.abs(xi) <= rad).all() and (rad > 0).all()
    assert len({tuple(col) for col in xi.T}) == xi.shape[1]                  # no two streams coincide


def test_fold_is_the_mean_plus_z_xi():
    idx, val, P, groups, K, q = _problem(2)
    S, w = 5, K + q
    xi = npd.normals(99, K, groups, q, S)
    Pd = npd.fold(P, groups, K, q, S, xi)
    assert Pd.shape == (P.shape[0], groups * q * S)
    draws = npd.cols(idx, val, Pd, 0, Pd.shape[1])
    for g, c, t in itertools.product(range(groups), range(q), range(S)):
        col = (g * q + c) * S + t
        Z = npd.cols(idx, val, P, g * w, K)
        mean = npd.cols(idx, val, P, g * w + K + c, 1)[:, 0]
        want = mean + Z @ xi[:, col]
        scale = np.abs(mean) + np.abs(Z) @ np.abs(xi[:, col])
        assert (np.abs(draws[:, col] - want) <= 64 * 2.0 ** -53 * scale).all()
    # columns do not depend on S
    Pd2 = npd.fold(P, groups, K, q, S + 2, npd.normals(99, K, groups, q, S + 2))
    for gc, t in itertools.product(range(groups * q), range(S)):
        np.testing.assert_array_equal(Pd2[:, gc * (S + 2) + t], Pd[:, gc * S + t])
