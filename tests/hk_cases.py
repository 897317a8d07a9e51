"""Helpers of the heat-kernel panel edge tests (test_hk_case_table.py on the CPU, test_gpu_hk_edges.py on the GPU).  Pure
Python and numpy; torch is imported only where a buffer goes to the device.

* the dispatch of flgp_dev_hk restated (csrc/gemm.hip, hk_panel2_applicable in csrc/hk2.hip, hk_panel_applicable in
  csrc/hk.hip): nks(), na(), route(); vw_elems() is the rule the workspace must obey.
* hk2_facts() / hk_facts(): what hk_panel2_kernel and hk_panel_kernel branch on for one case -- panels per workgroup, the
  ragged last panel and how it arrives, tile pairs / m-tiles per wave, ring parities, F and pf_at.
* place() / place_result(): an operand as a column-major block with a leading dimension larger than its row count, at a
  row offset, inside NaN (the columns k >= K included); a result inside canaries.
* the case tables.  test_hk_case_table.py asserts with the facts that they reach every edge they are there for.

Every tabled shape is tiny (n0 <= 7 * 64, n1 <= 545, K <= 288): the kernels take them with hk_panel_min_n0 = 0, the two
min_n1 keys at 1 and hk_panel_grid = the case's grid, so that a workgroup walks several panels.
"""
from __future__ import annotations

import numpy as np

HP = 64                                # rows of V0 per panel, both kernels
WAVES = 8
HK_MAX_NST = 18
LDS_MI355X = 160 * 1024                # dynamic LDS a workgroup may have on the device the tables are written for
CANARY_BITS = 0x7FF8C0DEFACE0BAD       # a quiet NaN with a payload: compared bit for bit
DEFAULTS = {"hk_panel": 1, "hk_panel2": 1, "hk_panel_min_n0": 2048, "hk_panel_min_n1": 64, "hk_panel2_min_n1": 480,
            "hk_panel_grid": 0}


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------- the dispatch, restated
def nks(K):
    """hk2_nks: the k steps (of 4) of the hk_panel2_kernel instance for K, 0 where there is none"""
    ks = (K + 3) // 4
    if ks > 52 or ks < 23:
        return 0
    if ks >= 47:
        return 52
    if ks > 28:
        return 0
    return 28 if ks > 26 else 26


def na(n):
    """hk2_na: the k steps of the panel's A part (two LDS copies)"""
    return 28 if n == 28 else 26


def ceil16(K):
    return ceil_div(K, 16) * 16


def n1p32(n1):
    return ceil_div(n1, 32) * 32


def vw_elems(n1, K):
    """doubles the scaled small operand needs in either layout: hk.hip pads K to 16, hk2.hip to 4 nks(K)"""
    return n1p32(n1) * max(ceil16(K), 4 * nks(K))


def route(n0, n1, K, ldh, tuning=None, lds=LDS_MI355X):
    """flgp_dev_hk_route: 2 = hk_panel2_kernel, 1 = hk_panel_kernel, 0 = the tiled GEMM"""
    t = dict(DEFAULTS, **(tuning or {}))
    n = nks(K)
    if n:
        slots = 2 * na(n) + (n - na(n))
        if (t["hk_panel"] and t["hk_panel2"] and n1 >= t["hk_panel2_min_n1"] and n0 >= t["hk_panel_min_n0"] and ldh <= 7000000
                and n1 <= 100000 and lds >= slots * 2048):
            return 2
    nst = ceil_div(K, 16)
    if (t["hk_panel"] and nst <= HK_MAX_NST and n1 >= t["hk_panel_min_n1"] and n0 >= t["hk_panel_min_n0"] and ldh <= 150000000
            and lds >= 8 * nst * 16 * HP):
        return 1
    return 0


def case_tuning(cs):
    """the keys a tabled case runs with"""
    return {"hk_panel_min_n0": 0, "hk_panel_min_n1": 1, "hk_panel2_min_n1": 1, "hk_panel_grid": cs["grid"]}


# ------------------------------------------------------------------------------------------------- what the kernels branch on
def panel_facts(n0, grid):
    """the persistent loop over panels, the same in both kernels"""
    panels = ceil_div(n0, HP)
    g = min(grid, panels) if grid > 0 else panels
    per_wg = [len(range(w, panels, g)) for w in range(g)]
    last_wg = (panels - 1) % g
    return {
        "panels": panels, "grid": g, "per_wg": per_wg, "rem": n0 % HP,
        "uneven": len(set(per_wg)) > 1,
        # the ragged last panel is not a workgroup's first: it comes in through the prefetch, not the prologue
        "ragged_by_prefetch": n0 % HP != 0 and per_wg[last_wg] > 1,
        # hk2's unconditional fetch: a workgroup's last panel fetches the matrix's last panel again -- its own (always so for
        # one workgroup), or, for some workgroup, another one's
        "refetch_other": any((w + (per_wg[w] - 1) * g) != panels - 1 for w in range(g)),
    }


def hk2_facts(n0, n1, K, grid):
    n = nks(K)
    assert n, "no hk_panel2_kernel instance for K = %d" % K
    f = panel_facts(n0, grid)
    npairs = ceil_div(n1, 32)
    ntw = [(npairs - w + WAVES - 1) // WAVES for w in range(WAVES)]
    odd = (n // 2) % 2 == 1
    tiles = set()                       # (last tile?, ring parity) over all waves
    for c in ntw:
        for t in range(c):
            tiles.add((t == c - 1, 1 if odd and t % 2 else 0))
    nb = n - na(n)
    f.update(nks=n, na=na(n), nb=nb, npairs=npairs, ntw=ntw, tiles=tiles,
             idle_waves=sum(1 for c in ntw if c == 0),
             # both LDS copies of the A part are written a second time: at least three panels in one workgroup
             a_copies_reused=max(f["per_wg"]) >= 3,
             tile_outside_n1=ceil_div(n1, 16) % 2 == 1,       # the second tile of the last pair starts at or past n1
             idle_wave_carries_next=any(c == 0 for c in ntw) and max(f["per_wg"]) >= 2)
    return f


def hk_facts(n0, n1, K, grid):
    nst = ceil_div(K, 16)
    assert nst <= HK_MAX_NST
    f = panel_facts(n0, grid)
    nmt = ceil_div(n1, 16)
    ntw = [(nmt - w + WAVES - 1) // WAVES for w in range(WAVES)]
    F = [c * nst for c in ntw]
    has_next = max(f["per_wg"]) >= 2
    f.update(nst=nst, PG=7 if nst <= 14 else 9, nmt=nmt, ntw=ntw, F=F, pf_at=[x - nst if x > nst else 0 for x in F],
             has_next=has_next,
             f0_with_next=has_next and any(x == 0 for x in F),
             fmod4_with_next={x % 4 for x in F if x > 0} if has_next else set(),
             # a wave with two m-tiles: the A ring's loads roll over into the next tile while the current one is multiplied;
             # with a stage count that is no multiple of the ring's four the tile also ends in the middle of a turn
             rollover_in_ring=any(c >= 2 for c in ntw),
             rollover_mid_turn=any(c >= 2 and nst % 4 for c in ntw))
    return f


# ------------------------------------------------------------------------------------------------- placement
class Placed:
    """A rows x K matrix as a column-major block inside a device buffer of NaN.  ptr: address of buffer element (0, 0), the
    argument dV0 / dV1 of flgp_dev_hk; the block's first row is row `off` of the buffer."""

    def __init__(self, buf, ld, off, rows, K):
        self.buf, self.ld, self.off, self.rows, self.K = buf, ld, off, rows, K
        self.ptr = buf.data_ptr()


def operand_host(a, pad_rows=3, off=5, pad_cols=None):
    """(host buffer (K + pad_cols) x ld with NaN outside the block, ld, off)"""
    rows, K = a.shape
    if pad_cols is None:
        pad_cols = max(ceil16(K), 4 * nks(K)) - K + 1      # every column a padded k loop could touch, and one more
    ld = off + rows + pad_rows
    host = np.full((K + pad_cols, ld), np.nan)
    host[:K, off:off + rows] = a.T
    return host, ld, off


def place(a, pad_rows=3, off=5, device="cuda"):
    """the matrix `a` (rows x K) on the device: leading dimension off + rows + pad_rows, first row at `off`, NaN in the rows
    before and behind it and in the columns k >= K"""
    import torch
    host, ld, off = operand_host(np.asarray(a, dtype=np.float64), pad_rows, off)
    return Placed(torch.from_numpy(host).to(device), ld, off, a.shape[0], a.shape[1])


class PlacedResult:
    """H (n0 x n1, column-major, ldh > n0) inside canaries: one whole column of them before, rows n0 .. ldh of every column,
    and one column behind"""

    def __init__(self, n0, n1, pad=5, device="cuda"):
        import torch
        self.n0, self.n1, self.ldh = n0, n1, n0 + pad
        host = np.full((n1 + 2, self.ldh), CANARY_BITS, dtype=np.int64).view(np.float64)
        self.buf = torch.from_numpy(host).to(device)
        self.ptr = self.buf.data_ptr() + 8 * self.ldh

    def read(self):
        """(H as n0 x n1, were all its elements written, are all canaries intact)"""
        host = self.buf.cpu().numpy()
        bits = host.view(np.int64)
        inside = bits[1:1 + self.n1, :self.n0]
        outside_ok = bool((bits[0] == CANARY_BITS).all() and (bits[-1] == CANARY_BITS).all()
                          and (bits[1:1 + self.n1, self.n0:] == CANARY_BITS).all())
        return host[1:1 + self.n1, :self.n0].T.copy(), bool((inside != CANARY_BITS).all()), outside_ok


def place_result(n0, n1, pad=5, device="cuda"):
    return PlacedResult(n0, n1, pad, device)


def rows_of(mode, n, rng):
    """(rows of the source matrix, index vector or None, rows of the source) for a logical operand of n rows:
    'range' -- the source is the operand; 'gather' -- a permuted subset of a source with 11 rows more; 'repeat' -- the same
    with one row taken twice"""
    if mode == "range":
        return np.arange(n), None, n
    ns = n + 11
    idx = rng.permutation(ns)[:n]
    if mode == "repeat" and n >= 2:
        idx[n - 1] = idx[0]
    return idx, idx.astype(np.int32), ns


# ------------------------------------------------------------------------------------------------- the tables
# A case: n0, the grid cap, n1, K, how the rows of V1 are named ('range' | 'gather' | 'repeat'), whether idx0 is a gather
def case(n0, grid, n1, K, idx1="range", gather0=False):
    return dict(n0=n0, grid=grid, n1=n1, K=K, idx1=idx1, gather0=gather0)


def case_id(cs):
    return "n0_%d-g%d-n1_%d-K%d-%s%s" % (cs["n0"], cs["grid"], cs["n1"], cs["K"], cs["idx1"], "-gather0" if cs["gather0"] else "")


# hk_panel2_kernel.  n0: 37 (one panel, n0 < 64), 128 (2, rem 0), 129 (3, rem 1), 191 (3, rem 63), 273 (5, rem 17),
# 447 (7, rem 63), 448 (7, rem 0), 81 (2, rem 17)
HK2_CASES = [
    case(37, 1, 20, 89, "range", True),
    case(128, 1, 33, 104, "repeat"),
    case(129, 1, 256, 105, "range"),
    case(273, 2, 257, 112, "repeat", True),
    case(447, 3, 520, 185, "range"),
    case(448, 3, 545, 208, "repeat"),
    case(273, 2, 545, 93, "range", True),
    case(447, 3, 520, 190, "repeat", True),
    case(191, 1, 20, 103, "range"),
    case(81, 1, 33, 190, "range", True),
    case(447, 3, 20, 112, "range"),
    case(273, 2, 20, 208, "repeat"),
    case(129, 1, 545, 104, "range"),
    case(448, 3, 257, 89, "repeat", True),
    case(129, 1, 256, 185, "range", True),
]

# hk_panel_kernel; every K outside hk2's ranges, so that the route is 1 with nothing switched off
HK_CASES = [
    case(37, 1, 1, 13, "range", True),
    case(128, 1, 16, 222, "repeat"),
    case(129, 1, 17, 239, "range"),
    case(273, 2, 128, 288, "repeat", True),
    case(447, 3, 129, 275, "range"),
    case(448, 3, 130, 222, "repeat"),
    case(273, 2, 1, 239, "range"),
    case(447, 3, 16, 13, "range", True),
    case(191, 1, 130, 13, "repeat"),
    case(81, 1, 17, 40, "range"),
    case(129, 1, 129, 239, "repeat", True),
    case(273, 2, 129, 40, "range"),
    case(128, 1, 129, 64, "range"),
]

# on both sides of every K at which the route changes (89, 104 | 105, 112, 185, 208 are in HK2_CASES)
ROUTE_K = (88, 113, 184, 209, 288, 289)
ROUTE_CASES = [case(129, 1, 33, K, "range", K % 2 == 0) for K in ROUTE_K]

# one multi-panel shape per kernel for the rounding bound
ROUNDING_HK2 = case(273, 2, 545, 190, "repeat", True)
ROUNDING_HK = case(273, 2, 130, 275, "repeat", True)
