"""The shapes of tests/test_gpu_predictor_pg_rows.py and a pure-Python model of how predictor_pg_rows_kernel
(csrc/predictor.hip) walks them, for tests/test_predictor_pg_case_table.py.  The kernel has one code path; what varies is

* the chunks a wave walks: chains [0, B) in 64-wide chunks, lane l of chunk c owning chain 64 c + l; the lanes of the last
  chunk that own a chain (its tail); how many lanes own no chain at all (they enter the butterfly with no candidate), one
  chain, or several (a running best over chunks);
* the rows of a workgroup (PRED_WAVES = 4 waves, a row each per step) and the number of workgroups;
* r: the row's pairs are broadcast from lanes 0 .. r-1 (r = 1 and r = FLGP_RMAX = 32 are the ends);
* which outputs are asked for: the link (exp) runs unless f alone is wanted; the butterfly only for a label."""
import itertools

NS = [1, 3, 4, 5, 257]
RS = [1, 5, 32]
SS = [1, 7, 300]
BS = [1, 2, 63, 64, 65, 130]
OUTPUTS = ("f", "pi", "y", "label")
SUBSETS = [c for k in range(1, 5) for c in itertools.combinations(OUTPUTS, k)]
PRED_WAVES, RMAX = 4, 32


def walk(B, outputs=OUTPUTS):
    chunks = (B + 63) // 64
    per_lane = [len(range(l, B, 64)) for l in range(64)]
    return dict(chunks=chunks, tail=B - 64 * (chunks - 1), idle_lanes=per_lane.count(0), one_chain_lanes=per_lane.count(1),
                many_chain_lanes=sum(1 for c in per_lane if c > 1), link=any(o != "f" for o in outputs),
                butterfly="label" in outputs)


def grid(n):
    blocks = min((n + PRED_WAVES - 1) // PRED_WAVES, 1 << 20)
    return dict(blocks=blocks, last_block_rows=n - PRED_WAVES * (blocks - 1))


def shapes(B):
    """the (r, s) the GPU test runs at B: all of them; every n of NS runs on each (a row's indices repeat where r > s)"""
    return [(r, s) for r in RS for s in SS]
