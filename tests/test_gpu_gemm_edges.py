"""GPU: csrc/gemm.hip's fp64 GEMM at its tile, stage, stride and reduction edges, against an EXACT reference.

Why the reference is exact.  A, B, E and E2 hold integers from [-8, 8]; alpha, beta and gamma come from {-3, 0.5, 2, 1, 0}.
Every product A(i,k) B(k,j) is an integer of magnitude <= 64, every partial sum of them -- in any order, over any k range,
on any split-K plane -- an integer of magnitude <= 64 Kd <= 64 * 5000 = 320000, and the epilogue's terms alpha * sum,
beta * E, gamma * E2 and their partial sums are multiples of 1/2 of magnitude <= 3 * 64 Kd + 3 * 8 + 3 * 8 < 10^6.  All of
these are far below 2^53 (2^52 for the halves), so every operation of the kernel is exact whatever its summation order, and
so is numpy's float64 `alpha * (A @ B) + beta * E + gamma * E2` (BLAS included, for the same reason).  The results are
compared with assert_array_equal: no tolerance.  The same holds for the fused reduction's unscaled modes: |S - I|^2 <=
(64 * 4098 + 1)^2 < 6.9e10 per element and < 4.6e15 < 2^53 over the 256^2 elements of the largest case.

Every operand lies in a larger buffer of NaN (gemm_cases.place): a kernel that multiplies padding by zero where it should
select it away gives NaN.  Every result lies in a buffer of canaries: each element outside the logical C must hold the
canary bit for bit afterwards, each element inside must have been written.

gemm_cases.plan restates the dispatch; test_gemm_case_table.py (CPU) shows with it that the tables below reach every path.
Here the launch's own plane count (info[0]) must agree with the plan's."""
import contextlib
import ctypes
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as G  # noqa: E402
from flgp_amd import _lib  # noqa: E402
from flgp_amd.pipeline import HipStages  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = G.CANARY_BITS
WORK_ELEMS = 2 * 1800 * 1700
LONGDOUBLE_OK = np.finfo(np.longdouble).nmant >= 63


@pytest.fixture(scope="module")
def stages():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    return HipStages(DEV)


@pytest.fixture(scope="module")
def work():
    return torch.full((WORK_ELEMS,), float("nan"), dtype=torch.float64, device=DEV)


@contextlib.contextmanager
def tuned(L, **keys):
    try:
        for k, v in keys.items():
            L.flgp_set_tuning(k.encode(), v)
        yield
    finally:
        for k, v in G.DEFAULTS.items():
            L.flgp_set_tuning(k.encode(), v)


def stream():
    return torch.cuda.current_stream().cuda_stream


def ints(rng, shape):
    return rng.integers(-8, 9, size=shape).astype(np.float64)


def gemm_ex(L, M, N, Kd, alpha, pA, pB, beta, pE, e_is, e_js, pC, work, work_elems, gamma=0.0, pE2=None, force_split=0,
            fused=None, pair=None, check=True):
    """pA: M x Kd, pB: N x Kd (B transposed), pC: M x N, all gemm_cases.Placed; fused = (mode, dinv, dist, scratch, counter)
    tensors; pair = (pA2, pB2, pC2).  Returns (rc, planes, fused_done)."""
    info = (ctypes.c_int * 2)(-1, -1)
    fm, fd = (-1, (None,) * 4) if fused is None else (fused[0], [None if t is None else t.data_ptr() for t in fused[1:]])
    p2 = (None, None, None) if pair is None else tuple(p.ptr for p in pair)
    rc = L.flgp_dev_gemm_ex(stream(), M, N, Kd, alpha, pA.ptr, pA.s0, pA.s1, pB.ptr, pB.s1, pB.s0, beta,
                            None if pE is None else pE.ptr, e_is, e_js, pC.ptr, pC.s0, pC.s1,
                            work.data_ptr() if work_elems else None, work_elems, gamma, None if pE2 is None else pE2.ptr,
                            force_split, fm, fd[0], fd[1], fd[2], fd[3], p2[0], p2[1], p2[2], info)
    if check:
        _lib.check(rc)
    torch.cuda.synchronize()
    return rc, info[0], info[1]


def run_case(L, cs, work):
    """one case of the tables against the exact reference; returns None or a message"""
    M, N, Kd = cs["M"], cs["N"], cs["Kd"]
    cid = G.case_id(cs)
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    p = G.case_plan(cs)
    a_is, a_ks, b_ks, b_js, c_is, c_js, e_is, e_js = G.case_strides(cs)
    A, B = ints(rng, (M, Kd)), ints(rng, (Kd, N))
    pA, pB = G.place(A, *cs["a"]), G.place(np.ascontiguousarray(B.T), *cs["b"])
    assert (pA.s0, pA.s1, pB.s1, pB.s0) == (a_is, a_ks, b_ks, b_js)
    ref = cs["alpha"] * (A @ B)
    ckind, cpad, coff = cs["c"]
    ekind = ("k" if ckind == "row" else "row") if "opp" in (cs["e"], cs["e2"]) else ckind
    pC = None
    terms = []
    for what, coef in ((cs["e"], cs["beta"]), (cs["e2"], cs["gamma"])):
        if what is None:
            terms.append(None)
        elif what == "nan":
            assert coef == 0.0
            terms.append(G.place(np.full((M, N), np.nan), ekind, cpad, coff))
        else:
            X = ints(rng, (M, N))
            ref = ref + coef * X
            if what == "C":
                assert ekind == ckind and pC is None
                pC = G.place(X, ckind, cpad, coff, fill_bits=CANARY)
                terms.append(pC)
            else:
                terms.append(G.place(X, ekind, cpad, coff))
    if pC is None:
        pC = G.place(None, ckind, cpad, coff, shape=(M, N), fill_bits=CANARY)
    pE, pE2 = terms
    assert (pC.s0, pC.s1) == (c_is, c_js) and all(t is None or (t.s0, t.s1) == (e_is, e_js) for t in terms)
    pair = None
    if cs["pair"]:
        A2, B2 = ints(rng, (M, Kd)), ints(rng, (Kd, N))
        pair = (G.place(A2, *cs["a"]), G.place(np.ascontiguousarray(B2.T), *cs["b"]),
                G.place(None, ckind, cpad, coff, shape=(M, N), fill_bits=CANARY))
        ref2 = cs["alpha"] * (A2 @ B2)
    _, planes, _ = gemm_ex(L, M, N, Kd, cs["alpha"], pA, pB, cs["beta"], pE, e_is, e_js, pC, work, cs["work"], cs["gamma"], pE2,
                           cs["force_split"], pair=pair)
    if planes != p["planes"]:
        return f"{cid}: the launch took {planes} planes, the plan says {p['planes']}"
    results = [("C", pC, ref)] + ([("C2", pair[2], ref2)] if pair else [])
    for name, pc, r in results:
        got = pc.read()
        if not np.array_equal(got, r):
            bad = np.argwhere(~(got == r))
            i, j = bad[0]
            return (f"{cid}: {name} differs from the exact reference at {len(bad)} of {r.size} elements, first ({i}, {j}): "
                    f"{got[i, j]!r} != {r[i, j]!r}  [tile {p['tile']}, swap {p['swap']}, planes {p['planes']}]")
        if not pc.outside_is(CANARY):
            return f"{cid}: a store outside the logical {name}"
    return None


def run_cases(L, cases, work):
    tiles = {cs["tile128"] for cs in cases}
    failures = []
    for t128 in sorted(tiles):
        with tuned(L, **({"gemm_tile64_below": 0} if t128 else {})):
            for cs in cases:
                if cs["tile128"] == t128:
                    msg = run_case(L, cs, work)
                    if msg:
                        failures.append(msg)
    assert not failures, f"{len(failures)} of {len(cases)} cases:\n" + "\n".join(failures[:20])


# ------------------------------------------------------------------------------------------------- the tables
@pytest.mark.parametrize("modes", G.RING_MODES)
@pytest.mark.parametrize("tile", [64, 128])
def test_stage_ring(stages, work, tile, modes):
    """one tile, every stage count of the list (0, 1, 2 stages; ns mod 3 = 0, 1, 2 on the FAST and the plain pipeline of the
    64-tile; ragged last stages with odd and even ends).  Kd = 0 gives exactly beta E + gamma E2."""
    run_cases(stages.L, G.stage_ring_cases(tile, modes), work)


@pytest.mark.parametrize("M", G.TILE_MN)
@pytest.mark.parametrize("tile", [64, 128])
def test_tiles(stages, work, tile, M):
    """M against every N of the list at Kd = 34: layouts, pads, offsets and epilogues cycle (pairwise complete, see
    test_gemm_case_table.py)"""
    run_cases(stages.L, G.tile_cases(tile, M), work)


@pytest.mark.parametrize("tile", [64, 128])
def test_tiles_named_shapes(stages, work, tile):
    """the heat-kernel call's shape (RC staging from an odd shifted row0), the four fast pairs on tiles that slid back, and
    every cause of the GEN staging on either operand"""
    run_cases(stages.L, G.tile_extra_cases(tile), work)


def test_default_dispatch_of_the_128_tile(stages, work):
    """no tuning key: 210 tiles of 128 take gemm_f64_kernel<128>, unsplit and in two planes"""
    one, two = G.default128_cases()
    assert (G.case_plan(one)["tile"], G.case_plan(one)["planes"]) == (128, 1)
    assert (G.case_plan(two)["tile"], G.case_plan(two)["planes"]) == (128, 2)      # run_case holds info[0] against this
    run_cases(stages.L, [one, two], work)


@pytest.mark.parametrize("tile", [64, 128])
def test_epilogue(stages, work, tile):
    """the four combinations of E and E2; beta = 0 / gamma = 0 with the term a buffer of NaN (never read); E in the opposite
    layout from C; C == E and C == E2 in place at ragged M, N >= tile, unsplit (no overlapping tiles) and split"""
    run_cases(stages.L, G.epilogue_cases(tile), work)


@pytest.mark.parametrize("tile", [64, 128])
def test_split_k(stages, work, tile):
    """Kd in {128, 1283, 5000} with a workspace, the launch's own split and force_split in {1, 2, 3, 7}: exact, and the
    launch's plane count is the plan's"""
    run_cases(stages.L, G.splitk_cases(tile), work)


@pytest.mark.parametrize("tile", [64, 128])
def test_pair(stages, work, tile):
    """two products in one launch, ragged, C column-major and row-major, the second with operands of its own: both exact"""
    run_cases(stages.L, G.pair_cases(tile), work)


@pytest.mark.parametrize("tile", [64, 128])
def test_force_split_beyond_the_workspace_is_refused(stages, work, tile):
    L = stages.L
    rng = np.random.default_rng(5)
    M, N, Kd = 130, 70, 1283
    pA, pB = G.place(ints(rng, (M, Kd)), "row", 0, 0), G.place(ints(rng, (N, Kd)), "row", 0, 0)
    pC = G.place(None, "row", 2, 1, shape=(M, N), fill_bits=CANARY)
    with tuned(L, **({"gemm_tile64_below": 0} if tile == 128 else {})):
        assert G.plan(M, N, Kd, 1, M, N, 1, 1, M + 2, work_elems=3 * M * N, force_split=4)["invalid"]
        rc, _, _ = gemm_ex(L, M, N, Kd, 1.0, pA, pB, 0.0, None, 0, 0, pC, work, 3 * M * N, force_split=4, check=False)
        assert rc == -1                                                    # FLGP_ERR_INVALID
        rc, _, _ = gemm_ex(L, M, N, Kd, 1.0, pA, pB, 0.0, None, 0, 0, pC, work, 0, force_split=2, check=False)
        assert rc == -1
    assert (pC.buf.cpu().numpy().view(np.int64) == CANARY).all()


def test_row_block_with_the_whole_products_split_has_its_bits(stages, work):
    """csrc/common.h on force_split: a row block of a product, given the whole product's plane count, adds every element's
    terms in the order the whole product does.  N(0,1) data, bit for bit; one block shorter than a tile."""
    L = stages.L
    M, N, Kd = 700, 40, 900
    rng = np.random.default_rng(700)
    pA = G.place(rng.normal(size=(M, Kd)), "row", 0, 0)
    pB = G.place(rng.normal(size=(N, Kd)), "k", 0, 0)
    pC = G.place(None, "row", 0, 0, shape=(M, N), fill_bits=CANARY)
    _, planes, _ = gemm_ex(L, M, N, Kd, 1.0, pA, pB, 0.0, None, 0, 0, pC, work, 64 * M * N)
    assert planes == G.plan(M, N, Kd, 1, M, 1, Kd, 1, M, work_elems=64 * M * N)["planes"] and planes > 1
    whole = pC.read()
    for r0, nb in ((0, 660), (660, 40)):
        pCb = G.place(None, "row", 0, 0, shape=(nb, N), fill_bits=CANARY)
        _, got_planes, _ = gemm_ex(L, nb, N, Kd, 1.0, pA.view(r0, nb), pB, 0.0, None, 0, 0, pCb, work, 64 * M * N, force_split=planes)
        assert got_planes == planes
        np.testing.assert_array_equal(pCb.read().view(np.int64), np.ascontiguousarray(whole[r0:r0 + nb]).view(np.int64))


# ------------------------------------------------------------------------------------------------- the fused reduction
def fused_buffers(b):
    nt1 = G.ceil_div(b, 16)
    dinv = torch.from_numpy(np.full(b, CANARY, dtype=np.int64).view(np.float64)).to(DEV)
    dist = torch.from_numpy(np.full(G.DIST_PARTS, CANARY, dtype=np.int64).view(np.float64)).to(DEV)
    scratch = torch.full((nt1 * nt1,), float("nan"), dtype=torch.float64, device=DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    return dinv, dist, scratch, counter


def bits(t):
    return t.cpu().numpy().view(np.int64)


def check_fused(mode, S, got_C, bufs, kernel_i_is_col, exact, where):
    """C, dinv, dist and the counter after a fused reduction of the product S (caller's rows and columns)"""
    dinv, dist, _, counter = bufs
    b = S.shape[0]
    ref_C, ref_dinv = G.fused_reference(S, mode)
    np.testing.assert_array_equal(got_C, ref_C, err_msg=f"{where}: C (mode {mode})")
    if mode & 1:
        np.testing.assert_array_equal(dinv.cpu().numpy(), ref_dinv, err_msg=f"{where}: dinv")
    else:
        assert (bits(dinv) == CANARY).all(), f"{where}: dinv written without bit 0"
    if mode & 4:
        # the documented order: the halving tree inside a tile, then tile q into part q mod 32 with q ascending
        ref_dist = G.fused_dist(ref_C, kernel_i_is_col)
        got = dist.cpu().numpy()
        if exact:       # integer terms: exact in any order
            np.testing.assert_array_equal(got, ref_dist, err_msg=f"{where}: dist (mode {mode})")
        else:
            # non-negative terms: two summation orders of n terms differ by at most (n - 1) 2^-52 of their sum (twice the
            # (n - 1) u bound of one order, u = 2^-53); n = b^2 bounds the terms of every part
            assert (np.abs(got - ref_dist) <= b * b * 2.0 ** -52 * ref_dist).all(), f"{where}: dist (mode {mode})"
    else:
        assert (bits(dist) == CANARY).all(), f"{where}: dist written without bit 2"
    assert int(counter.cpu()[0]) == 0, f"{where}: the counter is not back at zero"


def fused_operands(b, Kd, scaled, seed):
    """S = At Bt^T with At, Bt: b x Kd.  scaled: A == B with one all-zero column of A, so that S_jj = 0 gives dinv = 0"""
    rng = np.random.default_rng(seed)
    At = ints(rng, (b, Kd))
    if scaled:
        At[b // 3] = 0.0
        Bt = At
    else:
        Bt = ints(rng, (b, Kd))
    return At, Bt


@pytest.mark.parametrize("c_kind", ["row", "k"], ids=["C-column-major", "C-row-major"])
@pytest.mark.parametrize("b", G.FUSED_B)
def test_fused_reduction_through_the_gemm(stages, work, b, c_kind):
    """S = A^T B (A != B, so a swap of upper and lower shows), Kd = 1280 in planes, every mode of the fused reduction: C exact
    with the masked triangle's zeros in the caller's own rows and columns, dist exact in the documented order, the counter
    back at zero, a second call on the same counter the same bits.  Modes with bit 0: dinv exact (1 / sqrt of an exact
    integer, both correctly rounded), C = (v d_row) d_col exactly, dist within the summation bound."""
    L = stages.L
    Kd = G.FUSED_KD
    for scaled, modes in ((False, G.FUSED_PLAIN_MODES), (True, G.FUSED_SCALED_MODES)):
        At, Bt = fused_operands(b, Kd, scaled, b)
        S = At @ Bt.T
        pA, pB = G.place(At, "k", 0, 0), G.place(Bt, "k", 0, 0)
        for mode in modes:
            pC = G.place(None, c_kind, 3 if mode == 2 else 0, 0, shape=(b, b), fill_bits=CANARY)
            bufs = fused_buffers(b)
            where = f"b {b}, {'scaled' if scaled else 'plain'}"
            _, planes, done = gemm_ex(L, b, b, Kd, 1.0, pA, pB, 0.0, None, 0, 0, pC, work, 64 * b * b, fused=(mode,) + bufs)
            assert planes > 1 and done == 1, where
            check_fused(mode, S, pC.read(), bufs, c_kind == "row", not scaled, where)
            assert pC.outside_is(CANARY)
            first = [bits(pC.buf).copy(), bits(bufs[0]).copy(), bits(bufs[1]).copy()]
            _, _, done = gemm_ex(L, b, b, Kd, 1.0, pA, pB, 0.0, None, 0, 0, pC, work, 64 * b * b, fused=(mode,) + bufs)
            assert done == 1
            for x, y in zip(first, [bits(pC.buf), bits(bufs[0]), bits(bufs[1])]):
                np.testing.assert_array_equal(x, y, err_msg=f"{where}: second call, mode {mode}")
            assert int(bufs[3].cpu()[0]) == 0


@pytest.mark.parametrize("c_kind", ["row", "k"])
def test_fused_request_that_cannot_be_served_leaves_the_plain_product(stages, work, c_kind):
    """alpha != 1, or no workspace (no split): info[1] == 0, C is the plain product, nothing else is written"""
    L = stages.L
    b, Kd = 100, G.FUSED_KD
    At, Bt = fused_operands(b, Kd, False, 11)
    S = At @ Bt.T
    pA, pB = G.place(At, "k", 0, 0), G.place(Bt, "k", 0, 0)
    for alpha, welems in ((2.0, 64 * b * b), (1.0, 0)):
        pC = G.place(None, c_kind, 2, 1, shape=(b, b), fill_bits=CANARY)
        bufs = fused_buffers(b)
        _, planes, done = gemm_ex(L, b, b, Kd, alpha, pA, pB, 0.0, None, 0, 0, pC, work, welems, fused=(1 | 2 | 4,) + bufs)
        assert done == 0 and (planes > 1) == (welems > 0)
        np.testing.assert_array_equal(pC.read(), alpha * S)
        assert pC.outside_is(CANARY) and (bits(bufs[0]) == CANARY).all() and (bits(bufs[1]) == CANARY).all()
        assert int(bufs[3].cpu()[0]) == 0


@pytest.mark.parametrize("s,b", G.GRAM_FUSED_SB)
def test_fused_reduction_through_the_gram_kernel(stages, work, s, b):
    """csrc/rot.hip's Gram kernel with gemm.hip's reductions behind it (the eigensolver's route at even s): the plain
    reduction (flgp_dev_gram_small) exact on integer data, and every fused mode as above"""
    L = stages.L
    welems = 64 * b * b
    for scaled, modes in ((False, (None,) + G.FUSED_PLAIN_MODES), (True, G.FUSED_SCALED_MODES)):
        At, Bt = fused_operands(b, s, scaled, s + b)                     # tensor (b, s) == column-major s x b
        S = At @ Bt.T
        dA = torch.from_numpy(At).to(DEV)
        dB = dA if scaled else torch.from_numpy(Bt).to(DEV)
        for mode in modes:
            out = torch.from_numpy(np.full((b, b), CANARY, dtype=np.int64).view(np.float64)).to(DEV)
            where = f"s {s}, b {b}, {'scaled' if scaled else 'plain'}"
            if mode is None:
                _lib.check(L.flgp_dev_gram_small(stream(), s, b, dA.data_ptr(), dB.data_ptr(), out.data_ptr(), work.data_ptr(), welems))
                torch.cuda.synchronize()
                np.testing.assert_array_equal(out.cpu().numpy().T, S, err_msg=where)
                continue
            bufs = fused_buffers(b)
            for _ in range(2):                                           # (the second call: the counter was left at zero)
                _lib.check(L.flgp_dev_gram_small_fused(stream(), s, b, dA.data_ptr(), dB.data_ptr(), out.data_ptr(), work.data_ptr(), welems,
                                                       mode, *(t.data_ptr() for t in bufs)))
                torch.cuda.synchronize()
                check_fused(mode, S, out.cpu().numpy().T, bufs, True, not scaled, where)


# ------------------------------------------------------------------------------------------------- rounding
@pytest.mark.skipif(not LONGDOUBLE_OK, reason="np.longdouble has fewer than 63 mantissa bits here: no reference finer than float64")
@pytest.mark.parametrize("M,N,Kd,welems", [(130, 257, 33, 0), (64, 64, 5000, 64 * 64 * 64)])
@pytest.mark.parametrize("tile", [64, 128])
def test_rounding_on_normal_data(stages, work, tile, M, N, Kd, welems):
    """N(0,1) data against np.longdouble.  The bound is the elementwise (Kd + 4) 2^-53 (|alpha| |A| |B| + |beta| |E| +
    |gamma| |E2|): Kd roundings of the fused multiply-add chain in any order (planes included), one for alpha, two per
    epilogue term -- not a measured number."""
    L = stages.L
    rng = np.random.default_rng(M + N + Kd)
    A, B, E, E2 = rng.normal(size=(M, Kd)), rng.normal(size=(Kd, N)), rng.normal(size=(M, N)), rng.normal(size=(M, N))
    alpha, beta, gamma = 0.75, -1.25, 0.5
    ld = np.longdouble
    ref = ld(alpha) * (A.astype(ld) @ B.astype(ld)) + ld(beta) * E.astype(ld) + ld(gamma) * E2.astype(ld)
    bound = ld(Kd + 4) * ld(2.0) ** -53 * (abs(alpha) * (np.abs(A).astype(ld) @ np.abs(B).astype(ld)) + abs(beta) * np.abs(E).astype(ld)
                                           + abs(gamma) * np.abs(E2).astype(ld))
    with tuned(L, **({"gemm_tile64_below": 0} if tile == 128 else {})):
        for (ak, bk, ck) in (("row", "k", "row"), ("k", "row", "k")):
            pA, pB = G.place(A, ak, 2, 0), G.place(np.ascontiguousarray(B.T), bk, 2, 0)
            pE, pE2 = G.place(E, ck, 3, 1), G.place(E2, ck, 3, 1)
            pC = G.place(None, ck, 3, 1, shape=(M, N), fill_bits=CANARY)
            _, planes, _ = gemm_ex(L, M, N, Kd, alpha, pA, pB, beta, pE, pE.s0, pE.s1, pC, work, welems, gamma, pE2)
            assert (planes > 1) == (welems > 0)
            err = np.abs(pC.read().astype(ld) - ref)
            print(f"tile {tile} {M}x{N}x{Kd} planes {planes}: max err / bound = {float((err / bound).max()):.3f}")
            assert (err <= bound).all()
            assert pC.outside_is(CANARY)
