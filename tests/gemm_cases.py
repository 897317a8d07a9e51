"""Helpers of the f64 GEMM edge tests (test_gemm_case_table.py on the CPU, test_gpu_gemm_edges.py on the GPU).

* place(): a logical matrix inside a larger device buffer -- row-contiguous or k-contiguous, a leading dimension that is
  tight, even or odd, a base that is 16-byte aligned or 8 bytes off -- with NaN everywhere outside the matrix, or (for a
  result) a canary bit pattern everywhere.  A kernel that multiplies padding by zero where it should select it away then
  fails loudly, and a store outside an edge tile changes a canary.
* plan(): a pure-Python restatement of the dispatch of csrc/gemm.hip (gemm_launch, gemm_plan_split, make_operand and the
  head of gemm_f64_kernel): which tile, which staging per operand and tile, whether edge tiles slide back, the split-K planes
  and their stage counts, which planes run the FAST pipeline.  features() turns a plan into the set of paths it takes.
* the case tables the GPU tests run.  test_gemm_case_table.py asserts with plan() that they reach every path there is.
"""
from __future__ import annotations

import itertools

import numpy as np

GB, GK = 128, 16                       # csrc/gemm.hip: the large tile, the k depth of a stage
DEFAULTS = {"gemm_tile64_below": 200, "gemm_tile64_blocks": 256, "gemm_min_stages": 5}
CANARY_BITS = 0x7FF8C0DEFACE0BAD       # a quiet NaN with a payload: compared bit for bit, and poison if it is ever read
PADS, OFFSETS = (0, 2, 3), (0, 1)


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------- placement
def layout(shape, kind, pad, offset):
    """(stride of the first index, stride of the second index, buffer length) of a matrix of `shape` whose first index
    ('row') or second index ('k') is contiguous, with leading dimension = contiguous extent + pad, based `offset` doubles in."""
    r, c = shape
    assert kind in ("row", "k") and pad in PADS and offset in OFFSETS
    if kind == "row":
        ld = r + pad
        return 1, ld, offset + ld * c + 2
    ld = c + pad
    return ld, 1, offset + ld * r + 2


class Placed:
    """A logical matrix inside a device buffer (torch, float64).  ptr: address of element (0, 0)."""

    def __init__(self, buf, shape, s0, s1, offset):
        self.buf, self.shape, self.s0, self.s1, self.offset = buf, shape, s0, s1, offset
        self.ptr = buf.data_ptr() + 8 * offset

    def _index(self):
        r, c = self.shape
        return self.offset + np.arange(r)[:, None] * self.s0 + np.arange(c)[None, :] * self.s1

    def read(self):
        return self.buf.cpu().numpy()[self._index()]

    def outside_is(self, bits):
        """every element outside the logical matrix still holds `bits`"""
        host = self.buf.cpu().numpy().view(np.int64).copy()
        host[self._index().ravel()] = bits
        return bool((host == bits).all())

    def view(self, r0, nr):
        """rows [r0, r0 + nr) of the same buffer"""
        return Placed(self.buf, (nr, self.shape[1]), self.s0, self.s1, self.offset + r0 * self.s0)


def place(a, i_stride_kind, pad, offset, shape=None, fill_bits=None, device="cuda"):
    """The matrix `a` (rows x k) in a larger device buffer: i_stride_kind 'row' (rows contiguous) or 'k' (k contiguous),
    leading dimension = contiguous extent + pad, base shifted by `offset` doubles; NaN outside the matrix.
    a = None with `shape` and fill_bits: a result buffer, every element the canary."""
    import torch
    shape = a.shape if a is not None else shape
    s0, s1, size = layout(shape, i_stride_kind, pad, offset)
    if fill_bits is None:
        host = np.full(size, np.nan)
    else:
        host = np.full(size, fill_bits, dtype=np.int64).view(np.float64)
    if a is not None:
        r, c = shape
        host[offset + np.arange(r)[:, None] * s0 + np.arange(c)[None, :] * s1] = a
    buf = torch.from_numpy(host).to(device)
    assert buf.data_ptr() % 16 == 0, "the allocator's base is the aligned base of the tables"
    return Placed(buf, shape, s0, s1, offset)


# ------------------------------------------------------------------------------------------------- the dispatch, restated
def plan_split(M, N, Kd, work_elems, tune):
    """gemm_plan_split"""
    if M <= 0 or N <= 0:
        return 1
    gbt = 64 if ceil_div(M, GB) * ceil_div(N, GB) < tune["gemm_tile64_below"] else GB
    ntiles = ceil_div(M, gbt) * ceil_div(N, gbt)
    per = M * N
    nsplit = 1
    if ntiles < 256 and Kd >= 8 * GK:
        nsplit = min((tune["gemm_tile64_blocks"] if gbt == 64 else 512) // ntiles, Kd // (tune["gemm_min_stages"] * GK))
        if nsplit * per > work_elems:
            nsplit = work_elems // per
        nsplit = max(nsplit, 1)
    klen = ceil_div(ceil_div(max(Kd, 1), nsplit), GK) * GK
    return ceil_div(max(Kd, 1), klen)


def _operand_mode(rs, ks, al16, row0, nrows, gbt):
    """make_operand: (mode, why it is GEN)"""
    inside = row0 + gbt <= nrows
    if inside and al16 and rs == 1 and ks % 2 == 0:
        return "RC", None
    if inside and al16 and ks == 1 and rs % 2 == 0:
        return "KC", None
    if not inside:
        return "GEN", "edge"
    if (rs == 1 and ks % 2 == 0) or (ks == 1 and rs % 2 == 0):
        return "GEN", "unaligned"
    return "GEN", "odd"


def plan(M, N, Kd, a_is, a_ks, b_ks, b_js, c_is, c_js, a_al16=True, b_al16=True, aliased=False, has_e=False, has_e2=False,
         work_elems=0, force_split=0, pair=False, tune=None):
    """What gemm_launch does with the call.  has_e / has_e2: after beta == 0 / gamma == 0 dropped the term;
    aliased: C is one of the terms that are left."""
    tune = dict(DEFAULTS, **(tune or {}))
    out = {"invalid": False}
    swap = c_is == 1 and c_js != 1
    if swap:
        gM, gN = N, M
        opa = (b_js, b_ks, b_al16)         # (row stride, k stride, aligned) of the kernel's A
        opb = (a_is, a_ks, a_al16)
    else:
        gM, gN = M, N
        opa = (a_is, a_ks, a_al16)
        opb = (b_js, b_ks, b_al16)
    gbt = 64 if ceil_div(gM, GB) * ceil_div(gN, GB) < tune["gemm_tile64_below"] else GB
    per = gM * gN
    nsplit = plan_split(M, N, Kd, work_elems, tune) if (work_elems > 0 and not pair) else 1
    if force_split > 0:
        if pair or (force_split > 1 and (work_elems == 0 or force_split * per > work_elems)):
            out["invalid"] = True
            return out
        nsplit = force_split
    klen = ceil_div(ceil_div(max(Kd, 1), nsplit), GK) * GK
    planes = ceil_div(max(Kd, 1), klen)
    shift = planes > 1 or not aliased
    zs = []
    for z in range(planes):
        kbeg = z * klen
        kend = min(kbeg + klen, Kd)
        zs.append({"kbeg": kbeg, "kend": kend, "ns": max(0, ceil_div(kend - kbeg, GK))})
    tiles = []
    for tm in range(ceil_div(gM, gbt)):
        for tn in range(ceil_div(gN, gbt)):
            row0, col0 = tm * gbt, tn * gbt
            srow = scol = False
            if shift:
                if row0 + gbt > gM and gM >= gbt:
                    row0, srow = gM - gbt, True
                if col0 + gbt > gN and gN >= gbt:
                    col0, scol = gN - gbt, True
            ma, ca = _operand_mode(opa[0], opa[1], opa[2], row0, gM, gbt)
            mb, cb = _operand_mode(opb[0], opb[1], opb[2], col0, gN, gbt)
            fast = [gbt == 64 and z["ns"] > 0 and z["kend"] % 2 == 0 and z["kend"] - z["kbeg"] >= 2 and ma != "GEN" and mb != "GEN"
                    for z in zs]
            tiles.append({"row0": row0, "col0": col0, "shift_row": srow, "shift_col": scol, "a": ma, "a_why": ca, "b": mb,
                          "b_why": cb, "inside": row0 + gbt <= gM and col0 + gbt <= gN, "fast": fast,
                          "edge_row": tm * gbt + gbt > gM, "edge_col": tn * gbt + gbt > gN})
    epi = "planes" if planes > 1 else ("E+E2" if has_e and has_e2 else "E" if has_e else "E2" if has_e2 else "none")
    out.update(swap=swap, tile=gbt, gM=gM, gN=gN, shift_edges=shift, aliased=aliased, planes=planes, klen=klen, z=zs, tiles=tiles,
               epilogue=epi)
    return out


def features(p):
    """the paths of csrc/gemm.hip a planned call takes, as a set of tuples that start with the tile size"""
    f = set()
    if p["invalid"]:
        return f
    t = p["tile"]
    for tl in p["tiles"]:
        if tl["a"] != "GEN" and tl["b"] != "GEN":
            f.add((t, "modes", tl["a"], tl["b"]))
        for op in ("a", "b"):
            if tl[op] == "GEN":
                f.add((t, "gen", op, tl[op + "_why"]))
        for z, fast in zip(p["z"], tl["fast"]):
            if t == 64:
                f.add((t, "fast" if fast else "plain", "ns%3", z["ns"] % 3))
            if z["ns"] <= 2:
                f.add((t, "ns", z["ns"]))
            if z["kend"] > z["kbeg"] and (z["kend"] - z["kbeg"]) % GK:
                f.add((t, "ragged stage", "kend even" if z["kend"] % 2 == 0 else "kend odd"))
        for edge, sh, x0, n in ((tl["edge_row"], tl["shift_row"], tl["row0"], p["gM"]), (tl["edge_col"], tl["shift_col"], tl["col0"], p["gN"])):
            if sh:
                f.add((t, "shifted", "odd" if x0 % 2 else "even"))
            elif edge:
                f.add((t, "not shifted", "smaller than a tile" if n < t else "aliased"))
        f.add((t, "epilogue", p["epilogue"], "inside" if tl["inside"] else "edge"))
    f.add((t, "planes", min(p["planes"], 3)))
    if p["planes"] > 1 and p["z"][-1]["kend"] - p["z"][-1]["kbeg"] < p["klen"]:
        f.add((t, "ragged last plane"))
    return f


def required_features():
    """every combination that exists, per tile size"""
    req = set()
    for t in (64, 128):
        req |= {(t, "modes", a, b) for a in ("RC", "KC") for b in ("RC", "KC")}
        req |= {(t, "gen", op, why) for op in ("a", "b") for why in ("odd", "unaligned", "edge")}
        req |= {(t, "ns", n) for n in (0, 1, 2)}
        req |= {(t, "ragged stage", k) for k in ("kend even", "kend odd")}
        req |= {(t, "shifted", "even"), (t, "shifted", "odd"), (t, "not shifted", "smaller than a tile"), (t, "not shifted", "aliased")}
        req |= {(t, "epilogue", e, w) for e in ("planes", "none", "E", "E2", "E+E2") for w in ("inside", "edge")}
        req |= {(t, "planes", n) for n in (1, 2, 3)} | {(t, "ragged last plane")}
    req |= {(64, kind, "ns%3", m) for kind in ("fast", "plain") for m in (0, 1, 2)}
    return req


# ------------------------------------------------------------------------------------------------- cases
# A case is a dict: M, N, Kd; a / b / c = (kind, pad, offset) with kind 'row' | 'k' -- A is placed as M x Kd, B as its
# transpose N x Kd (so 'row' means j-contiguous), C as M x N ('row' = column-major, 'k' = row-major); e / e2: None, 'own'
# (a buffer of its own with C's layout), 'opp' (its own, the opposite layout; E2 shares E's strides), 'C' (in place), 'nan'
# (its own, all NaN, with a zero coefficient); alpha, beta, gamma; work: workspace doubles (0: none); force_split;
# tile128: gemm_tile64_below = 0; pair.
def case(M, N, Kd, a=("row", 0, 0), b=("row", 0, 0), c=("row", 0, 0), e=None, e2=None, alpha=0.5, beta=-3.0, gamma=2.0,
         work=0, force_split=0, tile128=False, pair=False, tag=""):
    return dict(M=M, N=N, Kd=Kd, a=a, b=b, c=c, e=e, e2=e2, alpha=alpha, beta=beta, gamma=gamma, work=work,
                force_split=force_split, tile128=tile128, pair=pair, tag=tag)


def case_id(cs):
    lay = "".join(f"{k[0]}{p}{o}" for k, p, o in (cs["a"], cs["b"], cs["c"]))
    return (f"{cs['M']}x{cs['N']}x{cs['Kd']}-{lay}-e{cs['e']}-e2{cs['e2']}-w{cs['work']}-f{cs['force_split']}"
            f"-t{128 if cs['tile128'] else 64}{'-pair' if cs['pair'] else ''}{'-' + cs['tag'] if cs['tag'] else ''}")


def case_tune(cs):
    return {"gemm_tile64_below": 0} if cs["tile128"] else {}


def case_strides(cs):
    """(a_is, a_ks, b_ks, b_js, c_is, c_js, e_is, e_js) of the call a case makes"""
    M, N, Kd = cs["M"], cs["N"], cs["Kd"]
    a_is, a_ks, _ = layout((M, Kd), *cs["a"])
    b_js, b_ks, _ = layout((N, Kd), *cs["b"])
    c_is, c_js, _ = layout((M, N), *cs["c"])
    e_is, e_js = c_is, c_js
    if "opp" in (cs["e"], cs["e2"]):
        e_is, e_js, _ = layout((M, N), "k" if cs["c"][0] == "row" else "row", cs["c"][1], cs["c"][2])
    return a_is, a_ks, b_ks, b_js, c_is, c_js, e_is, e_js


def case_plan(cs):
    a_is, a_ks, b_ks, b_js, c_is, c_js, _, _ = case_strides(cs)
    has_e = cs["e"] is not None and cs["beta"] != 0.0
    has_e2 = cs["e2"] is not None and cs["gamma"] != 0.0
    aliased = (has_e and cs["e"] == "C") or (has_e2 and cs["e2"] == "C")
    return plan(cs["M"], cs["N"], cs["Kd"], a_is, a_ks, b_ks, b_js, c_is, c_js, a_al16=cs["a"][2] == 0, b_al16=cs["b"][2] == 0,
                aliased=aliased, has_e=has_e, has_e2=has_e2, work_elems=cs["work"], force_split=cs["force_split"], pair=cs["pair"],
                tune=case_tune(cs))


def _kc_pad(Kd):
    return 3 if Kd % 2 else 0          # a k-contiguous operand keeps the KC staging only with an even row stride


RING_KD = (0, 1, 2, 3, 15, 16, 17, 18, 31, 32, 33, 34, 47, 48, 50, 64, 66, 81, 96, 98)
RING_MODES = ("RC-RC", "RC-KC", "KC-RC", "KC-KC", "GEN-RC")


def stage_ring_cases(tile, modes):
    """M = N = the tile, one staging pair, every Kd of the ring; C row-major (no orientation swap), E and E2 present"""
    out = []
    for Kd in RING_KD:
        ma, mb = modes.split("-")
        lay = {"RC": ("row", 0, 0), "KC": ("k", _kc_pad(Kd), 0), "GEN": ("row", 0, 1)}
        out.append(case(tile, tile, Kd, a=lay[ma], b=lay[mb], c=("k", 0, 0), e="own", e2="own", tile128=tile == 128, tag=modes))
    return out


TILE_MN = (1, 17, 63, 64, 65, 127, 128, 129, 130, 193, 257)
LAYOUTS8 = tuple(itertools.product(("row", "k"), repeat=3))
PADOFF = tuple(itertools.product(PADS, OFFSETS))
EPI4 = ((None, None), ("own", None), (None, "own"), ("own", "own"))


def tile_cases(tile, M):
    """one M against every N at Kd = 34: the eight layouts, pad x offset of every operand and the four epilogues cycle
    through the table with periods that are pairwise coprime or offset, so that every (layout, pad, offset) pair of two
    operands occurs -- test_gemm_case_table.py checks what the table reaches"""
    out = []
    mi = TILE_MN.index(M)
    for ni, N in enumerate(TILE_MN):
        q = mi * len(TILE_MN) + ni
        la, lb, lc = LAYOUTS8[q % 8]
        pa, pb, pc = PADOFF[q % 6], PADOFF[(q // 6 + q) % 6], PADOFF[(q // 36 + q // 2) % 6]
        e, e2 = EPI4[(q // 8 + q) % 4]
        out.append(case(M, N, 34, a=(la, *pa), b=(lb, *pb), c=(lc, *pc), e=e, e2=e2, tile128=tile == 128))
    return out


def tile_extra_cases(tile):
    """the shapes the cycling above cannot be trusted to hit, named: the heat-kernel call (an odd row count, an even leading
    dimension, an aligned base: RC staging from an odd shifted row0), the four fast staging pairs on shifted tiles, and every
    cause of the GEN staging on either operand"""
    t128 = tile == 128
    out = [case(129 + tile, 130, 34, a=("row", 3 if (129 + tile) % 2 else 2, 0), b=("row", 0, 0), c=("row", 2, 0), tile128=t128,
                tag="hk: RC from an odd shifted row0")]
    for la, lb in itertools.product((("row", 2, 0), ("k", 2, 0)), repeat=2):     # the four fast pairs on tiles that slid back
        out.append(case(tile + 2, 2 * tile + 2, 34, a=la, b=lb, c=("k", 0, 0), e="own", e2="own", tile128=t128, tag="fast pair, shifted"))
    for op in ("a", "b"):
        for why, lay in (("odd", ("row", 3, 0)), ("unaligned", ("row", 2, 1)), ("odd-k", ("k", 3, 0)), ("unaligned-k", ("k", 0, 1))):
            kw = {op: lay}
            out.append(case(2 * tile, 2 * tile, 34, c=("k", 0, 0), tile128=t128, tag=f"GEN {op} {why}", **kw))
    return out


def default128_cases():
    return [case(1800, 1700, 40, a=("row", 0, 0), b=("k", 0, 0), c=("row", 0, 0), e="own", tag="default dispatch"),
            case(1800, 1700, 176, a=("k", 0, 0), b=("row", 0, 0), c=("k", 0, 0), e="own", e2="own", work=2 * 1800 * 1700,
                 tag="default dispatch, two planes")]


def _ragged(tile):
    return (130, 70) if tile == 64 else (257, 130)


def epilogue_cases(tile):
    M, N = _ragged(tile)
    t128 = tile == 128
    W = 16 * M * N
    out = []
    for c in (("row", 2, 0), ("k", 3, 1)):
        for e, e2 in EPI4:
            out.append(case(M, N, 34, c=c, e=e, e2=e2, tile128=t128, tag="terms"))
        out.append(case(M, N, 34, c=c, e="nan", e2="own", beta=0.0, tile128=t128, tag="beta 0: E is not read"))
        out.append(case(M, N, 34, c=c, e="own", e2="nan", gamma=0.0, tile128=t128, tag="gamma 0: E2 is not read"))
        out.append(case(M, N, 1283, c=c, e="nan", e2="nan", beta=0.0, gamma=0.0, work=W, tile128=t128, tag="zero coefficients, split"))
        out.append(case(M, N, 34, c=c, e="opp", tile128=t128, tag="E in the opposite layout"))
        out.append(case(M, N, 34, c=c, e="opp", e2="opp", tile128=t128, tag="E and E2 in the opposite layout"))
        for work, Kd in ((0, 34), (0, 1283), (W, 1283)):
            out.append(case(M, N, Kd, c=c, e="C", beta=1.0, alpha=-3.0, work=work, tile128=t128, tag="C == E"))
            out.append(case(M, N, Kd, c=c, e="own", e2="C", gamma=1.0, work=work, tile128=t128, tag="C == E2"))
            out.append(case(M, N, Kd, c=c, e="C", e2="own", beta=0.5, work=work, tile128=t128, tag="C == E, with E2"))
    return out


SPLIT_KD = (128, 1283, 5000)
FORCE = (0, 1, 2, 3, 7)


def splitk_cases(tile):
    t128 = tile == 128
    out = []
    for (M, N), lay in (((64, 64), dict(a=("row", 0, 0), b=("k", 0, 0), c=("row", 0, 0))),
                        ((130, 70), dict(a=("k", 3, 1), b=("row", 2, 0), c=("k", 2, 1))),
                        ((17, 70), dict(a=("row", 3, 0), b=("k", 0, 0), c=("row", 0, 1))),       # (planes from tiles that stay edge tiles
                        ((2 * tile + 1, tile), dict(a=("row", 3, 0), b=("row", 0, 0), c=("k", 0, 0)))):  #  and from tiles that slide back inside)
        for Kd in SPLIT_KD:
            for fs in FORCE:
                for e, e2 in ((None, None), ("own", "own")):
                    lay2 = dict(lay)
                    if lay2["a"][0] == "k" and fs in (2, 3):
                        lay2["a"] = ("k", _kc_pad(Kd), 0)          # (some of the split cases on the KC staging)
                    out.append(case(M, N, Kd, e=e, e2=e2, work=64 * M * N, force_split=fs, tile128=t128, **lay2))
    return out


PAIR_SHAPES = ((333, 70, 40), (130, 257, 33))


def pair_cases(tile):
    return [case(M, N, Kd, a=("row", 0, 0), b=("row", 0, 0) if cl == "row" else ("k", 3, 0), c=(cl, pad, 0), alpha=al, pair=True,
                 tile128=tile == 128)
            for (M, N, Kd) in PAIR_SHAPES for cl, pad, al in (("row", 0, 1.0), ("k", 0, 2.0), ("row", 3, -3.0), ("k", 2, 0.5))]


def all_plain_cases():
    """every case that goes through the exact-reference runner"""
    out = []
    for tile in (64, 128):
        for modes in RING_MODES:
            out += stage_ring_cases(tile, modes)
        for M in TILE_MN:
            out += tile_cases(tile, M)
        out += tile_extra_cases(tile) + epilogue_cases(tile) + splitk_cases(tile) + pair_cases(tile)
    return out + default128_cases()


# ------------------------------------------------------------------------------------------------- the fused reduction
FUSED_B = (16, 40, 100, 256)
FUSED_KD = 1280
FUSED_PLAIN_MODES = (0, 2, 8, 4, 2 | 4, 8 | 4)
FUSED_SCALED_MODES = (1, 1 | 4, 1 | 2 | 4)
GRAM_FUSED_SB = ((256, 64), (258, 128), (1030, 192), (4098, 256))
DIST_PARTS = 32


def fused_reference(S, mode):
    """GemmFusedReduce (csrc/common.h) on the product S, in the caller's own rows and columns: (C, dinv)"""
    b = S.shape[0]
    C = S.astype(np.float64).copy()
    dinv = None
    if mode & 1:
        d = np.diag(S)
        dinv = np.where(d > 0.0, 1.0 / np.sqrt(np.where(d > 0.0, d, 1.0)), 0.0)
        C = (C * dinv[:, None]) * dinv[None, :]          # (v d_row) d_col
    r, c = np.indices((b, b))
    if mode & 2:
        C[r >= c] = 0.0
    if mode & 8:
        C[r <= c] = 0.0
    return C, dinv


def fused_dist(C, kernel_i_is_col):
    """The 32 parts of |C - I|_F^2, added in the documented order: inside a 16 x 16 tile the halving tree over its 256 terms
    (the term of the kernel's (i, j) at leaf 16 (i % 16) + j % 16), then tile q into part q mod 32 with q ascending.
    kernel_i_is_col: the kernel's i runs over the caller's columns (a column-major result)."""
    b = C.shape[0]
    K = C.T if kernel_i_is_col else C                    # K[i, j] in the kernel's own indices
    D = (K - np.eye(b)) ** 2
    nt1 = ceil_div(b, 16)
    P = np.zeros((nt1 * 16, nt1 * 16))
    P[:b, :b] = D
    parts = np.zeros(DIST_PARTS)
    for q in range(nt1 * nt1):
        i0, j0 = (q // nt1) * 16, (q % nt1) * 16
        red = P[i0:i0 + 16, j0:j0 + 16].ravel().copy()
        off = 128
        while off:
            red[:off] += red[off:2 * off]
            off >>= 1
        parts[q % DIST_PARTS] += red[0]
    return parts
