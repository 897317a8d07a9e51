"""GPU (-m gpu): Gram with its columns dealt to the waves longest first (flgp_dev_gram_order + flgp_dev_gram_ordered,
csrc/sparse.hip).  Which wave takes which column changes no sum, so G must be flgp_dev_gram's bit for bit -- and the
oracle's, on the crafted patterns of test_gpu_gram_blocks.py (a hub column that holds every row, columns of 0, 1, RPG - 1
and RPG entries, fillers) -- for every lanes-per-row instance of the kernel, with and without windows, with ldg > s.

The list itself is an exact sort: descending entry count, ties by ascending column.  "Bucket width" 1: the counts along
the list never increase, and the list is numpy's stable argsort of the negated counts.  The kernel keeps no keys in LDS and
has one route for every s: a workgroup ranks 64 columns, each of its sixteen waves against ceil(s / 16) of the keys, so the
s below sit around one and several workgroups and around shares of one key, of none (s < 16) and of many."""
import functools

import numpy as np
import pytest
import torch

import np_sparse_stages as nps
from flgp_amd.pipeline import HipStages
from test_gpu_gram_blocks import crafted, reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BUCKET_WIDTH = 1                 # the order is exact: counts[order] is non-increasing, not only to within a bucket
RS = [1, 6, 10, 11, 12, 13, 16, 17, 21, 22, 32]      # r lanes per row: 1..12 and 17..21; 16: 13..16; 32: 22..32
RECORD_RS = RS                   # records of 128 bytes up to r = 10, of 256 up to 21, of 384 beyond


@pytest.fixture(scope="module")
def stages():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    return HipStages(DEV)


def gram(stages, d_idx, d_val, s, csc, order, pad=3, window=0, rec=None):
    """G (s x (s + pad), the padding NaN) from flgp_dev_gram (order is None) or flgp_dev_gram_ordered (a device list)"""
    n, r = d_idx.shape
    ldg = s + pad
    G = torch.full((s, ldg), float("nan"), dtype=torch.float64, device=DEV)
    L = stages.L
    L.flgp_set_tuning(b"sparse_window", window)
    try:
        if order is None:
            rc = L.flgp_dev_gram(stages._st(), d_idx.data_ptr(), d_val.data_ptr(), n, s, r, csc["colptr"].data_ptr(),
                                 csc["pos"].data_ptr(), G.data_ptr(), ldg)
        else:
            rc = L.flgp_dev_gram_ordered(stages._st(), d_idx.data_ptr(), d_val.data_ptr(), n, s, r, csc["colptr"].data_ptr(),
                                         csc["pos"].data_ptr(), order.data_ptr(), rec.data_ptr() if rec is not None else None,
                                         G.data_ptr(), ldg)
        torch.cuda.synchronize()
    finally:
        L.flgp_set_tuning(b"sparse_window", 0)
    assert rc == 0, L.flgp_last_error()
    return G


def expected_order(counts):
    return np.argsort(-np.asarray(counts, dtype=np.int64), kind="stable").astype(np.int32)


def check_order(order, counts):
    s = len(counts)
    assert np.array_equal(np.sort(order), np.arange(s))                                 # a permutation of 0..s-1
    along = np.asarray(counts)[order]
    assert (along[1:] <= along[:-1] + (BUCKET_WIDTH - 1)).all()                         # the longest columns lead
    assert np.array_equal(order, expected_order(counts))                                # ties by ascending column


# ------------------------------------------------------------------------------------------------------ G, crafted patterns
@pytest.mark.parametrize("window", [0, 16])
@pytest.mark.parametrize("r", RS)
def test_ordered_gram_is_the_plain_gram_and_the_oracles(stages, r, window):
    idx, val, s = crafted(r)
    d_idx, d_val = torch.from_numpy(idx).to(DEV), torch.from_numpy(val).to(DEV)
    csc = stages.csc(d_idx, s)
    counts = np.bincount(idx.ravel(), minlength=s)
    check_order(csc["order"].cpu().numpy(), counts)
    G_plain = gram(stages, d_idx, d_val, s, csc, None, window=window)
    G_order = gram(stages, d_idx, d_val, s, csc, csc["order"], window=window)
    assert torch.equal(G_order[:, :s], G_plain[:, :s])
    assert torch.isnan(G_order[:, s:]).all(), "the padding past s was written"
    np.testing.assert_array_equal(G_order[:, :s].cpu().numpy(), reference(r))
    if window == 0:                                                                     # shortest first: any permutation will do
        G_rev = gram(stages, d_idx, d_val, s, csc, torch.flip(csc["order"], [0]).contiguous())
        assert torch.equal(G_rev[:, :s], G_plain[:, :s])


def records(stages, d_idx, d_val):
    n, r = d_idx.shape
    rec = torch.full((stages.L.flgp_dev_gram_record_bytes(n, r) // 8,), float("nan"), dtype=torch.float64, device=DEV)
    assert rec.data_ptr() % 128 == 0
    rc = stages.L.flgp_dev_gram_pack(stages._st(), d_idx.data_ptr(), d_val.data_ptr(), n, r, rec.data_ptr())
    assert rc == 0, stages.L.flgp_last_error()
    return rec


@pytest.mark.parametrize("window", [0, 16])
@pytest.mark.parametrize("r", RECORD_RS)
def test_gram_from_row_records(stages, r, window):
    """the operands of a visit read from the row's record (values, then indices, on a 128-byte boundary): the same bits"""
    idx, val, s = crafted(r)
    d_idx, d_val = torch.from_numpy(idx).to(DEV), torch.from_numpy(val).to(DEV)
    csc = stages.csc(d_idx, s)
    G = gram(stages, d_idx, d_val, s, csc, csc["order"], window=window, rec=records(stages, d_idx, d_val))
    np.testing.assert_array_equal(G[:, :s].cpu().numpy(), reference(r))
    assert torch.isnan(G[:, s:]).all(), "the padding past s was written"
    assert torch.equal(d_idx.cpu(), torch.from_numpy(idx)) and torch.equal(d_val.cpu(), torch.from_numpy(val))   # the ELL arrays stay


@pytest.mark.parametrize("r", [10, 16, 32])
def test_ordered_gram_through_the_stage(stages, r):
    """HipStages.gram: the list of HipStages.csc, and records where flgp_dev_gram_uses_records says so (one window)"""
    idx, val, s = crafted(r)
    d_idx, d_val = torch.from_numpy(idx).to(DEV), torch.from_numpy(val).to(DEV)
    assert stages.L.flgp_dev_gram_uses_records(s, r) == 1 and stages.L.flgp_dev_gram_uses_records(20001, r) == 0
    np.testing.assert_array_equal(stages.gram(d_idx, d_val, stages.csc(d_idx, s)).cpu().numpy(), reference(r))
    assert torch.equal(d_idx.cpu(), torch.from_numpy(idx)) and torch.equal(d_val.cpu(), torch.from_numpy(val))


def test_ordered_gram_with_nothing_but_ties(stages):
    """sixty columns of thirty entries each and five that no row references: the list is the identity"""
    from oracle import flgp_oracle as O
    O.build()
    n, r, s = 600, 3, 65
    rng = np.random.default_rng(11)
    i = np.arange(n)
    idx = np.stack([i % 20, 20 + (7 * i) % 20, 40 + (3 * i) % 20], axis=1).astype(np.int32)
    val = rng.normal(size=(n, r)) * 2.0 ** rng.integers(-40, 41, size=(n, r))
    counts = np.bincount(idx.ravel(), minlength=s)
    assert (counts[:60] == 30).all() and (counts[60:] == 0).all()
    d_idx, d_val = torch.from_numpy(idx).to(DEV), torch.from_numpy(val).to(DEV)
    csc = stages.csc(d_idx, s)
    assert np.array_equal(csc["order"].cpu().numpy(), np.arange(s))
    G_plain = gram(stages, d_idx, d_val, s, csc, None)
    G_order = gram(stages, d_idx, d_val, s, csc, csc["order"])
    assert torch.equal(G_order[:, :s], G_plain[:, :s])
    np.testing.assert_array_equal(G_order[:, :s].cpu().numpy(), O.gram(idx, val, s))
    assert (G_order[60:, :s] == 0.0).all()


def test_ordered_gram_in_two_windows(stages):
    """s = 20001 is the first s whose row of G no longer fits one workgroup's LDS (windows of 16384 columns)"""
    n, r, s = 3000, 10, 20001
    idx, val, _ = nps.ell_inputs(n, s, r, seed=5, with_sizes=False)
    d_idx, d_val = torch.from_numpy(idx).to(DEV), torch.from_numpy(val).to(DEV)
    csc = stages.csc(d_idx, s)
    check_order(csc["order"].cpu().numpy(), np.bincount(idx.ravel(), minlength=s))
    G_plain = gram(stages, d_idx, d_val, s, csc, None, pad=1)
    G_order = gram(stages, d_idx, d_val, s, csc, csc["order"], pad=1)
    assert torch.equal(G_order[:, :s], G_plain[:, :s])
    assert torch.isnan(G_order[:, s:]).all()
    assert torch.equal(G_order[:, :s], G_order[:, :s].t())


# ------------------------------------------------------------------------------------------------------ the list itself
@functools.lru_cache(maxsize=None)
def column_counts(s):
    """few distinct counts (many ties), some empty columns, one hub"""
    rng = np.random.default_rng([3, s])
    counts = rng.integers(0, 6, size=s) * rng.integers(0, 4, size=s)
    counts[rng.integers(0, s)] = 100000
    return counts.astype(np.int64)


@pytest.mark.parametrize("s", [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 4100])
def test_order_list(stages, s):
    counts = column_counts(s)
    colptr = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(DEV)
    lists = []
    for _ in range(2):
        buf = torch.full((s + 1,), -7, dtype=torch.int32, device=DEV)
        rc = stages.L.flgp_dev_gram_order(stages._st(), colptr.data_ptr(), s, buf.data_ptr())
        torch.cuda.synchronize()
        assert rc == 0, stages.L.flgp_last_error()
        assert int(buf[s]) == -7, "the list was written past s"
        lists.append(buf[:s].cpu().numpy())
    check_order(lists[0], counts)
    assert np.array_equal(lists[0], lists[1])                                           # two calls, one list
