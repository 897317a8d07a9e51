"""Plain numpy restatements of the sparse device stages between the k-NN list and the heat kernel
(flgp_amd/csrc/sparse.hip, flgp_amd/csrc/lae.hip), one rounded operation at a time: no `@`, no `sum()`, no `einsum`,
so that numpy cannot pick a summation order of its own.  tests/test_sparse_stage_restatements.py anchors them to the
compiled oracle on the CPU; tests/test_gpu_sparse_stages.py holds the kernels to them bit for bit.  The second half of
the file holds the inputs both test modules share."""
import math

import numpy as np

COLSUM_CHUNK = 1024      # rows per chunk of the two-level column sums (oracle/flgp_oracle.c, csrc/sparse.hip)
MEAN_SLAB = 4096         # elements per workgroup of slab_sum_kernel (csrc/lae.hip)


# ---------------------------------------------------------------------------------------------------------- restatements
def u_recover(idx, val, V, eig, scale, root=False, descending=False):
    """flgp_dev_u_recover: vectors(i, k) = ((sum_a val(i, a) V(idx(i, a), k)) / sigma_k) * scale with the sum started
    at 0.0 and walked in ascending a (multiply, then add), sigma = sqrt(max(eig, 0)); a column with sigma == 0 is exactly
    +0.0.  V is s x K.  Returns (vectors n x K, values K).  `descending` walks a the other way round: never what the
    kernels do, only the yardstick that shows a reordering changes bits on the shared inputs."""
    idx = np.asarray(idx); val = np.asarray(val, dtype=np.float64); V = np.asarray(V, dtype=np.float64)
    eig = np.asarray(eig, dtype=np.float64)
    n, r = idx.shape
    K = V.shape[1]
    acc = np.zeros((n, K))
    for a in (range(r - 1, -1, -1) if descending else range(r)):
        acc = acc + val[:, a, None] * V[idx[:, a], :]
    ev = np.where(eig > 0.0, eig, 0.0)                       # the kernels' `ev > 0.0 ? ev : 0.0`: -0.0 and NaN become +0.0
    sigma = np.sqrt(ev)
    out = np.zeros((n, K))
    pos = sigma > 0.0
    out[:, pos] = (acc[:, pos] / sigma[None, pos]) * np.float64(scale)
    return out, (sigma if root else ev)


def mean(x):
    """flgp_dev_mean: the fixed tree of slab_sum_kernel / final_mean_kernel.  Per slab of 4096 elements lane t adds
    x[base + 256 k + t] for k = 0..15 in order from 0.0 (elements past the end are skipped); the 256 lane sums are halved
    with strides 128, 64, ..., 1; the slab totals are added in order from 0.0 and divided by the count."""
    x = np.asarray(x, dtype=np.float64).ravel()
    count = x.size
    total = np.float64(0.0)
    for base in range(0, count, MEAN_SLAB):
        lane = np.zeros(256)
        for k in range(16):
            piece = x[base + 256 * k: min(base + 256 * (k + 1), base + MEAN_SLAB, count)]
            if piece.size:
                lane[:piece.size] = lane[:piece.size] + piece
        off = 128
        while off > 0:
            lane[:off] = lane[:off] + lane[off:2 * off]
            off >>= 1
        total = total + lane[0]
    return total / np.float64(count)


def colsum(idx, val, s):
    """flgp_dev_colsum: chunks of 1024 rows; inside a chunk a column's entries are added in entry order from 0.0, then
    the chunk totals in chunk order from 0.0."""
    idx = np.asarray(idx); val = np.asarray(val, dtype=np.float64)
    n = idx.shape[0]
    out = np.zeros(s)
    for i0 in range(0, n, COLSUM_CHUNK):
        part = np.zeros(s)
        np.add.at(part, idx[i0:i0 + COLSUM_CHUNK].ravel(), val[i0:i0 + COLSUM_CHUNK].ravel())   # unbuffered: entry order
        out = out + part
    return out


def col_scale(idx, val, colsum, num_class, mode):
    """col_scale_kernel.  mode 0: v * (1.0 / (c + 1e-9)), then * num_class[j] if given; mode 1: v * (1.0 / sqrt(|c| + 1e-9))."""
    idx = np.asarray(idx); val = np.asarray(val, dtype=np.float64)
    c = np.asarray(colsum, dtype=np.float64)[idx]
    if mode == 0:
        v = val * (1.0 / (c + 1e-9))
        if num_class is not None:
            v = v * np.asarray(num_class, dtype=np.float64)[idx]
        return v
    if mode == 1:
        return val * (1.0 / np.sqrt(np.abs(c) + 1e-9))
    raise ValueError(mode)


def row_normalize(val):
    """row_normalize_kernel: the row sum in ascending slot order from 0.0, inv = 1.0 / (rs + 1e-9), then inv * v."""
    val = np.asarray(val, dtype=np.float64)
    rs = np.zeros(val.shape[0])
    for a in range(val.shape[1]):
        rs = rs + val[:, a]
    inv = 1.0 / (rs + 1e-9)
    return inv[:, None] * val


def graph_laplacian(idx, val, s, gl, num_class=None):
    """graphLaplacian_cpp as the device runs it, in two passes: column sums and scaling (not for "rw"), then rows."""
    if gl != "rw":
        val = col_scale(idx, val, colsum(idx, val, s), num_class if gl == "cluster-normalized" else None, 0)
    return row_normalize(val)


# --------------------------------------------------------------------------------------------------------- shared inputs
# U-recovery shapes: (route, K, n, r, s, root, scale, want_values, seed).  route names the kernel the entry point picks:
# "null" = no workspace (u_recover_kernel: 8 columns x 256 rows per block), "tiled" = K odd (64 x 64 tile, 16 rows per
# wave in batches of 8), "kpl2" = K % 4 == 2 (128 columns x 64 rows), "kpl4" = K % 4 == 0 (256 columns x 32 rows, 8 per
# wave).  K and n sit on, one below and one above those tile edges; s walks the 32-wide tile of transpose_v_kernel.
# scale "sqrtn" is the path's sqrt(n), "third" is 1000 / 3 (not a power of two).  The seed of a case with r >= 3 is one
# for which walking a in descending order changes at least one bit (test_sparse_stage_restatements.py checks that).
U_RECOVER_CASES = [
    # route   K    n    r   s  root  scale   values seed
    ("null", 1, 1, 3, 31, 0, "third", True, 7),
    ("null", 7, 255, 3, 32, 1, "sqrtn", True, 0),
    ("null", 8, 256, 10, 33, 0, "third", True, 0),
    ("null", 9, 257, 32, 97, 1, "sqrtn", True, 0),
    ("null", 65, 257, 10, 97, 0, "third", False, 0),
    ("null", 65, 1, 10, 31, 1, "sqrtn", True, 0),
    ("null", 8, 255, 1, 32, 0, "third", True, 0),
    ("null", 7, 256, 32, 33, 1, "third", True, 0),
    ("null", 9, 255, 10, 31, 0, "sqrtn", True, 0),
    ("tiled", 1, 1, 10, 31, 0, "sqrtn", True, 1),
    ("tiled", 63, 7, 3, 32, 1, "third", True, 0),
    ("tiled", 65, 8, 10, 33, 0, "sqrtn", True, 0),
    ("tiled", 129, 9, 32, 97, 1, "third", True, 0),
    ("tiled", 1, 15, 1, 32, 0, "third", True, 0),
    ("tiled", 63, 16, 3, 31, 1, "sqrtn", False, 0),
    ("tiled", 65, 17, 10, 97, 0, "third", True, 0),
    ("tiled", 129, 63, 32, 33, 1, "sqrtn", True, 0),
    ("tiled", 1, 64, 3, 32, 0, "third", True, 0),
    ("tiled", 63, 65, 10, 31, 1, "third", True, 0),
    ("tiled", 65, 130, 32, 33, 0, "sqrtn", True, 0),
    ("tiled", 129, 130, 10, 97, 1, "third", True, 0),
    ("kpl2", 2, 1, 32, 32, 0, "third", True, 0),
    ("kpl2", 126, 63, 3, 31, 1, "sqrtn", True, 0),
    ("kpl2", 130, 64, 10, 33, 0, "third", True, 0),
    ("kpl2", 258, 65, 32, 97, 1, "sqrtn", False, 0),
    ("kpl2", 130, 130, 10, 32, 0, "third", True, 0),
    ("kpl2", 2, 130, 1, 31, 1, "sqrtn", True, 0),
    ("kpl2", 258, 1, 3, 33, 0, "third", True, 0),
    ("kpl4", 4, 1, 3, 31, 1, "third", True, 0),
    ("kpl4", 252, 7, 10, 32, 0, "sqrtn", True, 0),
    ("kpl4", 256, 8, 32, 33, 1, "third", True, 0),
    ("kpl4", 260, 9, 3, 97, 0, "sqrtn", True, 0),
    ("kpl4", 516, 31, 10, 31, 1, "third", False, 0),
    ("kpl4", 4, 32, 1, 32, 0, "sqrtn", True, 0),
    ("kpl4", 252, 33, 32, 33, 1, "sqrtn", True, 0),
    ("kpl4", 256, 33, 10, 97, 0, "third", True, 0),
    ("kpl4", 260, 70, 3, 32, 1, "third", True, 0),
    ("kpl4", 516, 70, 32, 97, 0, "sqrtn", True, 0),
]


def u_recover_case_id(case):
    route, K, n, r, s, root, scale, want_values, _ = case
    return f"{route}-K{K}-n{n}-r{r}-s{s}-root{root}-{scale}" + ("" if want_values else "-novalues")


def u_recover_route(K, workspace):
    if not workspace:
        return "null"
    return "kpl4" if K % 4 == 0 else "kpl2" if K % 2 == 0 else "tiled"


def u_recover_scale(kind, n):
    return math.sqrt(float(n)) if kind == "sqrtn" else 1000.0 / 3.0


def u_recover_inputs(K, n, r, s, seed):
    """idx random in [0, s) with anchor 0 in row 0 and anchor s - 1 in the last row (the last row wins where one slot
    has to hold both); val = normal x 10**uniform(-3, 3): mixed signs and magnitudes, so that a reordering of the sum
    changes bits; V random normal (s x K); eig descending and positive."""
    rng = np.random.default_rng([seed, K, n, r, s])
    idx = rng.integers(0, s, size=(n, r)).astype(np.int32)
    val = rng.normal(size=(n, r)) * 10.0 ** rng.uniform(-3.0, 3.0, size=(n, r))
    V = np.asfortranarray(rng.normal(size=(s, K)))
    eig = np.sort(rng.uniform(0.05, 1.0, size=K))[::-1].copy()
    if n:
        idx[0, 0] = 0
        idx[n - 1, r - 1] = s - 1
    return idx, val, V, eig


def ell_inputs(n, s, r, seed, with_sizes=True):
    """A random ELL matrix as the Laplacian stages see it: r distinct anchors per row in ascending order, positive
    weights over four orders of magnitude, and positive cluster sizes."""
    rng = np.random.default_rng([seed, n, s, r])
    idx = np.sort(rng.permuted(np.tile(np.arange(s, dtype=np.int32), (n, 1)), axis=1)[:, :r], axis=1)
    val = rng.uniform(0.1, 1.0, size=(n, r)) * 10.0 ** rng.uniform(-2.0, 2.0, size=(n, r))
    sizes = rng.integers(1, 50, size=s).astype(np.float64) if with_sizes else None
    return np.ascontiguousarray(idx), np.ascontiguousarray(val), sizes


def mean_inputs(count, seed=0):
    """Mixed signs over twelve orders of magnitude: any other association of the sum changes its last bits."""
    rng = np.random.default_rng([seed, count])
    return rng.normal(size=count) * 10.0 ** rng.uniform(-6.0, 6.0, size=count)


MEAN_COUNTS = [1, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 5]
