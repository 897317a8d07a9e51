"""The shapes of tests/test_gpu_predictor_cols.py and tests/test_gpu_predictor_draws_fold.py and a pure-Python model of how the
kernels of csrc/predictor_cols.hip walk them, for tests/test_predictor_draws_case_table.py.  What varies with the shape:

* flgp_dev_predictor_cols: calls narrower than the knob predictor_cols_tile_min (512) go to predictor_pg_rows_kernel, the
  same chain; the kernel tests set the knob to 1 so that every shape reaches the tile kernel, and serve ROUTED_NCS at the
  default;
* predictor_cols_kernel: a workgroup owns 64 rows x 64 columns (PC_TILE); the last row tile and the last column tile may be
  partial, and both at once; wave w of 4 computes rows 16 w .. 16 w + 15, so a partial row tile leaves whole waves idle; c0
  shifts the loads off a 64-column boundary (the tile edges are relative to c0, not to P);
* draws_fold_kernel: 256 columns of one group per workgroup (a partial last one), DF_J = 8 rows of P per pass (a partial last
  pass clamps its loads to row s - 1), a grid plane per group; K is the length of the chain;
* a draws handle over a Nystrom bandwidth: ncol <= 8 takes the mean-only route, ncol > 8 the columns-out route; features
  always take the columns-out route, with K columns."""
PC_TILE, PC_WAVES, DF_COLS, DF_J, NP_CM = 64, 4, 256, 8, 8
TILE_MIN = 512                                            # knob predictor_cols_tile_min: narrower calls go to predictor_pg_rows_kernel
ROUTED_NCS = [511, 512, 577]                              # widths served at the default knob: both kernels, and a partial tile

# flgp_dev_predictor_cols
NS = [1, 63, 64, 65, 257]
RS = [1, 5, 32]
SS = [1, 7, 300]
NCS = [1, 63, 64, 65, 130]
C0S = [0, 3, 64]

# the fold
FOLD_S = [1, 7, 300]
FOLD_K = [1, 63, 64, 65, 130]
FOLD_GQ = [(1, 1), (3, 1), (1, 3)]
FOLD_DRAWS = [1, 5, 64, 65]
FOLD_EXTRA = [(7, 5, (1, 3), 100)]                        # (s, K, (groups, q), S): 300 columns of one group, two workgroups


def tiles(n, nc, c0=0):
    rt, ct = (n + PC_TILE - 1) // PC_TILE, (nc + PC_TILE - 1) // PC_TILE
    last_rows, last_cols = n - PC_TILE * (rt - 1), nc - PC_TILE * (ct - 1)
    per_wave = PC_TILE // PC_WAVES
    return dict(row_tiles=rt, col_tiles=ct, last_rows=last_rows, last_cols=last_cols,
                partial_rows=last_rows < PC_TILE, partial_cols=last_cols < PC_TILE,
                idle_waves=PC_WAVES - (last_rows + per_wave - 1) // per_wave, aligned=c0 % PC_TILE == 0,
                first_tile_is_last=(rt == 1, ct == 1))


def cols_route(nc, tile_min=TILE_MIN):
    """the kernel flgp_dev_predictor_cols launches: "tile" (predictor_cols_kernel) or "pg_rows" (predictor_pg_rows_kernel, f alone)"""
    return "tile" if nc >= max(1, tile_min) else "pg_rows"


def fold_walk(s, K, groups, q, S):
    qS = q * S
    blocks = (qS + DF_COLS - 1) // DF_COLS
    passes = (s + DF_J - 1) // DF_J
    return dict(col_blocks=blocks, last_block_cols=qS - DF_COLS * (blocks - 1), passes=passes, last_pass_rows=s - DF_J * (passes - 1),
                planes=groups, chain=K, ncol=groups * qS, waves_in_last_block=(qS - DF_COLS * (blocks - 1) + 63) // 64)


def nystrom_route(kind, ncol):
    """the route a served block takes on a Nystrom handle: "mean" (nystrom_mean_rows, passes of NP_CM columns) or "cols\""""
    return "mean" if kind == "draws" and ncol <= NP_CM else "cols"


# the handle tests (tests/test_gpu_predictor_draws.py, tests/test_gpu_predictor_covariance.py): K of the handle, and
# (groups, q, S) of the draws made from it
HANDLE_K = [12, 20, 200]
HANDLE_DRAWS = [(1, 3, 2), (1, 3, 5), (1, 3, 30), (3, 1, 2), (3, 1, 22)]
BIT_ROWS = 513                                            # served as one call, in blocks of 256 and one at a time
