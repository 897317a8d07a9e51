"""CPU: the numpy restatement of the wave tiles (tests/np_row_tiles.py) against the layout as include/flgp_hip.h states it,
and unpack(pack(.)) returns the ELL arrays."""
import numpy as np
import pytest

import np_row_tiles as T


def test_pair_slots_and_sizes():
    assert [T.pair_slots(r) for r in (1, 2, 3, 10, 11, 12, 13, 24, 25, 32)] == [1, 1, 2, 5, 6, 6, 8, 12, 15, 18]
    assert T.tile_bytes(10) == 5 * 1536 and T.tile_bytes(10) % 128 == 0
    assert T.image_bytes(10000, 10) == 157 * 5 * 1536 and T.image_bytes(10048, 10) == 157 * 5 * 1536
    assert T.image_bytes(10049, 10) == 158 * 5 * 1536 and T.image_bytes(0, 10) == 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("r", [1, 3, 10, 11, 13, 25, 32])
def test_unpack_returns_the_rows(n, r):
    rng = np.random.default_rng([n, r])
    idx = rng.integers(1, 5000, size=(n, r)).astype(np.int32)
    val = rng.normal(size=(n, r))
    image = T.pack(idx, val)
    assert image.size == T.image_bytes(n, r)
    idx2, val2, pad_zero = T.unpack(image, n, r)
    assert np.array_equal(idx2, idx) and np.array_equal(val2, val) and pad_zero


def test_addresses_as_stated():
    """pair p of lane l of tile t: values at t TB + (p 64 + l) 16, indices at t TB + PT 1024 + (p 64 + l) 8"""
    n, r = 130, 13
    rng = np.random.default_rng(5)
    idx = rng.integers(1, 5000, size=(n, r)).astype(np.int32)
    val = rng.normal(size=(n, r))
    image = T.pack(idx, val)
    pt, tb = T.pair_slots(r), T.tile_bytes(r)
    for row, p in [(0, 0), (63, 6), (64, 3), (129, 6), (129, 7), (130, 0)]:
        t, l = divmod(row, 64)
        zo = t * tb + (p * 64 + l) * 16
        jo = t * tb + pt * 1024 + (p * 64 + l) * 8
        z = image[zo:zo + 16].view(np.float64)
        j = image[jo:jo + 8].view(np.int32)
        for h in range(2):
            a = 2 * p + h
            live = row < n and a < r
            assert z[h] == (val[row, a] if live else 0.0) and j[h] == (idx[row, a] if live else 0)
