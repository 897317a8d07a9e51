"""numpy restatement of the wave tiles of the ELL rows (csrc/sparse.hip, row_tiles_pack_kernel; include/flgp_hip.h).

Tile T holds rows 64 T .. 64 T + 63: first PT x 64 value pairs of 16 bytes, pair p of lane l at (p 64 + l) 16, then PT x 64
index pairs of 8 bytes in the same order.  Pair p of a row is its entries 2 p and 2 p + 1; slots past r and rows past n hold
value 0.0 and index 0.  PT = steps x NP with steps = ceil(ceil(r / 2) / 6) and NP = ceil(ceil(r / 2) / steps)."""
import numpy as np

MAX_PAIRS = 6
LANES = 64


def pair_slots(r):
    pairs = (r + 1) // 2
    steps = -(-pairs // MAX_PAIRS)
    return steps * -(-pairs // steps)


def tile_bytes(r):
    return pair_slots(r) * LANES * (16 + 8)


def image_bytes(n, r):
    return -(-n // LANES) * tile_bytes(r) if n > 0 else 0


def pack(idx, val):
    """the tile image of (idx, val), both n x r, as a uint8 array of image_bytes(n, r)"""
    n, r = idx.shape
    pt, nt = pair_slots(r), -(-n // LANES)
    v = np.zeros((nt * LANES, 2 * pt), dtype=np.float64)
    j = np.zeros((nt * LANES, 2 * pt), dtype=np.int32)
    v[:n, :r] = val
    j[:n, :r] = idx
    # (tile, lane, pair, half) -> (tile, pair, lane, half)
    v = np.ascontiguousarray(v.reshape(nt, LANES, pt, 2).transpose(0, 2, 1, 3)).reshape(nt, -1)
    j = np.ascontiguousarray(j.reshape(nt, LANES, pt, 2).transpose(0, 2, 1, 3)).reshape(nt, -1)
    return np.concatenate([v.view(np.uint8), j.view(np.uint8)], axis=1).reshape(-1)


def unpack(image, n, r):
    """(idx, val, padding_is_zero) of a tile image"""
    pt, nt = pair_slots(r), -(-n // LANES)
    t = np.asarray(image, dtype=np.uint8).reshape(nt, tile_bytes(r))
    v = np.ascontiguousarray(t[:, :pt * LANES * 16]).view(np.float64).reshape(nt, pt, LANES, 2)
    j = np.ascontiguousarray(t[:, pt * LANES * 16:]).view(np.int32).reshape(nt, pt, LANES, 2)
    v = v.transpose(0, 2, 1, 3).reshape(nt * LANES, 2 * pt)
    j = j.transpose(0, 2, 1, 3).reshape(nt * LANES, 2 * pt)
    pad_zero = (not v[n:].view(np.int64).any() and not j[n:].any() and not v[:n, r:].view(np.int64).any()
                and not j[:n, r:].any())
    return j[:n, :r].copy(), v[:n, :r].copy(), bool(pad_zero)
