"""gram_kernel at the edges of its schedule: rows per group, groups per step, steps per column, the positions fetched two
steps ahead -- bit for bit against oracle.gram, which sums every G(j1, j2) in ascending row order.

The pattern is crafted: a hub column that holds every row, fourteen named columns with exact entry counts (none, one,
around a group, around one, two and three blocks of 64 positions), and filler columns for the rest of each row.  The values
spread over many binades with both signs, so that another order of the sums changes bits; the tests without the `gpu` mark
prove that on the same inputs with a numpy restatement of the kernel's schedule."""
import functools

import numpy as np
import pytest
import torch

from flgp_amd.pipeline import HipStages

DEV = "cuda:0"
N_ROWS = 2100
N_FILL = 45                      # filler columns: at least r - 1 = 31 of them, s = 1 + 14 + 45 = 60
RS = [1, 2, 6, 7, 10, 11, 16, 17, 21, 22, 32]      # every packing, both sides of each change of 64 // r
WINDOWS = [0, 16, 24]            # all columns in one LDS table; windows of 16; of 24, which does not divide s


def schedule(r):
    """(rows per group, positions per step) of gram_kernel at this r: a group is 64 // r rows where that is more than the
    power-of-two packing holds (four rows up to r = 16, two above), and a step is 64 positions or as many as the groups in
    flight (11 with r lanes per row, 16 with 16 or 32) cover."""
    pow2 = 4 if r <= 16 else 2
    rpg, in_flight = (64 // r, 11) if 64 // r > pow2 else (pow2, 16)
    groups = -(-64 // rpg)
    return rpg, (64 if groups <= in_flight else in_flight * rpg)


def named_counts(r):
    rpg, _ = schedule(r)
    return [0, 1, rpg - 1, rpg, rpg + 1, 63, 64, 65, 127, 128, 129, 191, 192, 193]


@functools.lru_cache(maxsize=None)
def crafted(r):
    """(idx, val, s): column 0 is the hub, columns 1..14 have exactly named_counts(r) entries, the rest fill the rows up.
    At r = 1 a row has one entry, so the hub holds the rows the named columns leave over."""
    rng = np.random.default_rng([2024, r])
    counts = named_counts(r)
    s = 1 + len(counts) + N_FILL
    per_row = [[] for _ in range(N_ROWS)] if r == 1 else [[0] for _ in range(N_ROWS)]
    room = np.full(N_ROWS, 1 if r == 1 else r - 1)
    for k, c in enumerate(counts):
        rows = rng.choice(np.nonzero(room > 0)[0], size=c, replace=False)
        room[rows] -= 1
        for i in rows:
            per_row[i].append(1 + k)
    fillers = np.arange(1 + len(counts), s)
    idx = np.empty((N_ROWS, r), dtype=np.int32)
    for i, cols in enumerate(per_row):
        if r == 1:
            cols = cols or [0]
        else:
            cols = cols + list(rng.choice(fillers, size=r - len(cols), replace=False))
        idx[i] = np.sort(cols)
    val = rng.normal(size=(N_ROWS, r)) * 2.0 ** rng.integers(-40, 41, size=(N_ROWS, r))
    return idx, np.ascontiguousarray(val), s


@functools.lru_cache(maxsize=None)
def reference(r):
    from oracle import flgp_oracle as O
    O.build()
    idx, val, s = crafted(r)
    G = O.gram(idx, val, s)
    G.setflags(write=False)
    return G


def restated(idx, val, s, r, groups_reversed=False, rows_descending=False):
    """The kernel's schedule in numpy: a column's entries in ascending row order, cut into steps, a step into groups of rows;
    every product is multiplied, then added to its bin.  The two switches apply the groups of a step, or the rows of a group,
    in the opposite order."""
    rpg, step = schedule(r)
    G = np.zeros((s, s))
    order = np.argsort(idx.ravel(), kind="stable")                  # entries by column, rows ascending inside a column
    colptr = np.searchsorted(idx.ravel()[order], np.arange(s + 1))
    for j1 in range(s):
        entries = order[colptr[j1]:colptr[j1 + 1]]
        for p in range(0, len(entries), step):
            blk = entries[p:p + step]
            grp = [blk[g:g + rpg] for g in range(0, len(blk), rpg)]
            for g in (grp[::-1] if groups_reversed else grp):
                for e in (g[::-1] if rows_descending else g):
                    row = e // r
                    G[j1, idx[row]] += val.ravel()[e] * val[row]     # r distinct bins: one add each
    return G


# ------------------------------------------------------------------------------------------------- on the CPU
@pytest.mark.parametrize("r", RS)
def test_pattern_has_the_named_counts(r):
    idx, val, s = crafted(r)
    counts = np.bincount(idx.ravel(), minlength=s)
    assert list(counts[1:15]) == named_counts(r)
    assert counts[0] == (N_ROWS - sum(named_counts(r)) if r == 1 else N_ROWS)
    assert 40 <= s <= 70 and (np.diff(idx, axis=1) > 0).all()


@pytest.mark.parametrize("r", RS)
def test_only_the_ascending_order_gives_the_oracles_bits(r):
    idx, val, s = crafted(r)
    want = reference(r)
    np.testing.assert_array_equal(restated(idx, val, s, r), want)
    rpg, step = schedule(r)
    if step > rpg:                                                   # (at r = 1 the 64 rows of a step are one group)
        assert not np.array_equal(restated(idx, val, s, r, groups_reversed=True), want)
    assert rpg > 1
    assert not np.array_equal(restated(idx, val, s, r, rows_descending=True), want)


# ------------------------------------------------------------------------------------------------- on the GPU
@pytest.fixture(scope="module")
def stages():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    return HipStages(DEV)


@functools.lru_cache(maxsize=None)
def device_case(r):
    idx, val, s = crafted(r)
    return torch.from_numpy(idx).to(DEV), torch.from_numpy(val).to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("r", RS)
def test_gram_blocks_bit_exact(stages, r, window):
    """flgp_dev_gram itself, with ldg = s + 3: the padding is NaN before and after."""
    idx, val, s = crafted(r)
    d_idx, d_val = device_case(r)
    csc = stages.csc(d_idx, s)
    ldg = s + 3
    G = torch.full((s, ldg), float("nan"), dtype=torch.float64, device=DEV)
    stages.L.flgp_set_tuning(b"sparse_window", window)
    try:
        rc = stages.L.flgp_dev_gram(stages._st(), d_idx.data_ptr(), d_val.data_ptr(), N_ROWS, s, r, csc["colptr"].data_ptr(),
                                    csc["pos"].data_ptr(), G.data_ptr(), ldg)
        torch.cuda.synchronize()
    finally:
        stages.L.flgp_set_tuning(b"sparse_window", 0)
    assert rc == 0, stages.L.flgp_last_error()
    G = G.cpu().numpy()
    np.testing.assert_array_equal(G[:, :s], reference(r))
    np.testing.assert_array_equal(G[:, :s], G[:, :s].T)
    assert np.isnan(G[:, s:]).all(), "the padding past s was written"


@pytest.mark.gpu
@pytest.mark.parametrize("r", [10, 16, 32])
def test_gram_blocks_through_the_stage(stages, r):
    idx, val, s = crafted(r)
    d_idx, d_val = device_case(r)
    G = stages.gram(d_idx, d_val, stages.csc(d_idx, s)).cpu().numpy()
    np.testing.assert_array_equal(G, reference(r))
