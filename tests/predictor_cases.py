"""The shapes of tests/test_gpu_predictor_rows.py and a pure-Python model of how predictor_rows_kernel (csrc/predictor.hip)
walks them, for tests/test_predictor_case_table.py.  The kernel has one code path; what varies with the shape is

* the column chunks a wave walks: columns [j_lo, j_hi) of the group's K + q in 64-wide chunks c_lo .. c_hi - 1, where
  j_lo = 0 with a variance and K without, j_hi = K + q with a mean and K without;
* where the q mean columns sit: behind the last squares in the same chunk, alone in a chunk of their own, or across a
  chunk edge; and whether the last chunk is full or partial;
* the rows of a workgroup (PRED_WAVES = 4 waves, a row each per step) and the number of workgroups;
* r (the row's pairs are broadcast from lanes 0 .. r-1: r = 1 and r = FLGP_RMAX = 32 are the ends) and the groups."""
S = 40
KQ = [(1, 0), (1, 1), (62, 1), (63, 1), (64, 1), (127, 2), (200, 17)]
GROUPS = [1, 3]
RS = [1, 3, 10, 32]
NS = [1, 63, 64, 65, 257]
PRED_WAVES, RMAX = 4, 32


def walk(K, q, mean=True, var=True):
    """what one wave does for one (row, group): the chunk range, the lanes of the last chunk and where the mean sits"""
    w = K + q
    j_lo, j_hi = (0 if var else K), (w if mean else K)
    c_lo, c_hi = j_lo // 64, (j_hi + 63) // 64
    if not (mean and q):
        place = "none"
    elif K // 64 != (w - 1) // 64:
        place = "straddles"
    elif K % 64 == 0:
        place = "own chunk"
    else:
        place = "behind the squares"
    return dict(c_lo=c_lo, chunks=c_hi - c_lo, tail=j_hi - 64 * (c_hi - 1), place=place,
                square_terms_per_lane=(K + 63) // 64 if var else 0)


def grid(n, groups):
    blocks = min((n + PRED_WAVES - 1) // PRED_WAVES, 1 << 20)
    return dict(blocks=blocks, last_block_rows=n - PRED_WAVES * (blocks - 1), grid_y=min(groups, 65535))
