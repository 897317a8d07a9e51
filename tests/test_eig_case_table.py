"""CPU: the case tables of test_gpu_eig_edges.py reach every path flgp_dev_eig_topk picks from (s, K).

plan() (eig_cases.py) restates the decisions of csrc/eig.hip in Python; features() names the paths a plan takes.  The tables
must hold every row listed here and reach every feature of required_features(), so an edit of the tables cannot drop a path
without this file noticing.  (That plan() itself tells the truth is checked on the GPU, against flgp_dev_eig_plan, which is
computed by the functions the solve itself calls.)"""
import eig_cases as E

# (s, K): b, Jacobi kernel, block columns live -> padded, refinement (0 full Jacobi, 1 small64, 2 sub-Jacobi), g, kernel of the
# sub-Jacobi, rot.hip's products
TRUNCATED = {
    (257, 1): (32, 32, 2, 2, 0, 31, None, False),
    (258, 8): (32, 32, 2, 2, 0, 24, None, False),
    (300, 20): (48, 32, 3, 4, 1, 28, None, False),
    (301, 20): (48, 32, 3, 4, 1, 28, None, False),
    (420, 56): (80, 32, 5, 6, 1, 24, None, False),
    (640, 150): (192, 32, 12, 12, 1, 42, None, True),
    (641, 150): (192, 32, 12, 12, 1, 42, None, False),
    (700, 240): (304, 32, 19, 20, 1, 64, None, False),
    (700, 255): (320, 32, 20, 20, 2, 65, 0, False),
    (900, 320): (400, 32, 25, 26, 2, 80, 32, False),
    (900, 330): (416, 16, 52, 52, 2, 86, 0, False),
    (1100, 400): (512, 16, 64, 64, 2, 112, 32, False),
    (2300, 870): (1088, 16, 136, 136, 2, 218, 0, False),
    (2300, 880): (1104, -1, 69, 70, 2, 224, 32, False),
}
# s: Jacobi kernel, block-column width, block columns live -> padded
DENSE = {1: (0, 32, 1, 2), 2: (0, 32, 1, 2), 3: (0, 32, 1, 2), 16: (0, 32, 1, 2), 31: (0, 32, 1, 2), 32: (32, 16, 2, 2),
         48: (32, 16, 3, 4), 400: (32, 16, 25, 26), 416: (16, 8, 52, 52), 512: (16, 8, 64, 64), 528: (16, 8, 66, 66),
         1023: (0, 4, 256, 256), 1025: (-1, 16, 65, 66), 1088: (16, 8, 136, 136), 1104: (-1, 16, 69, 70)}


def feats(cases):
    got = set()
    for s, K in cases:
        got |= E.features(E.plan(s, K))
    return got


def test_tables_reach_every_path():
    missing = E.required_features() - feats(E.all_cases())
    assert not missing, sorted(missing, key=str)


def test_plan_restates_the_library():
    """flgp_dev_eig_plan launches nothing, so it answers without a GPU: on every case of the tables and on a sweep of (s, K)"""
    import ctypes
    from flgp_amd import _lib
    L = _lib.lib()
    cases = E.all_cases() + [(s, K) for s in list(range(1, 70)) + list(range(250, 2400, 37)) + [4096, 16384, 65536, 70000]
                             for K in sorted({1, 2, s // 7, s // 3, s // 2 - 40, s // 2, s - 1, s}) if 1 <= K <= s]
    out = (ctypes.c_int * 8)()
    for s, K in cases:
        _lib.check(L.flgp_dev_eig_plan(s, K, ctypes.addressof(out)))
        assert list(out) == E.plan_ints(E.plan(s, K)), (s, K)
    assert L.flgp_dev_eig_plan(10, 11, ctypes.addressof(out)) == -1 and L.flgp_dev_eig_plan(0, 0, ctypes.addressof(out)) == -1


def test_truncated_table():
    assert sorted(E.TRUNCATED_CASES) == sorted(TRUNCATED)
    for (s, K), (b, jac, live, nbc, refine, g, sub, rot) in TRUNCATED.items():
        p = E.plan(s, K)
        assert not p["dense"] and s > 2 * b and s > 256, (s, K)
        assert (p["b"], p["jac"], p["live"], p["nbc"], p["refine"], p["g"], p["rot"]) == (b, jac, live, nbc, refine, g, rot), (s, K)
        assert (p["sub"]["nloc"] if p["sub"] else None) == sub, (s, K)
        assert p["bs"] == (s >= 1536)
    # the sub-Jacobi of (900, 320) visits a padded block column of its own; both full-Jacobi cases are one workgroup, one round
    assert E.plan(900, 320)["sub"]["nbc"] == E.plan(900, 320)["sub"]["live"] + 1
    # b = 400 / 416 and 1088 / 1104 are neighbours across a kernel switch, 512 the last width of the register-staged load
    assert E.jacobi_plan(400)["nloc"] == 32 and E.jacobi_plan(416)["nloc"] == 16
    assert E.jacobi_plan(1088)["nloc"] == 16 and E.jacobi_plan(1104)["nloc"] == -1


def test_dense_table():
    assert sorted(E.DENSE_CASES) == sorted([(s, s) for s in DENSE] + [(416, 200)])
    for s, (jac, w, live, nbc) in DENSE.items():
        p = E.plan(s, s)
        assert p["dense"] and p["b"] == s and p["refine"] == 0 and not p["bs"] and not p["rot"]
        assert (p["jac"], p["w"], p["live"], p["nbc"]) == (jac, w, live, nbc), s
    p = E.plan(416, 200)                 # K < s, s > 256: dense only because 2b >= s
    assert p["dense"] and p["b"] == 416 and 2 * E.block_size(416, 200) >= 416 and p["jac"] == 16
    assert any(s % 2 for s in DENSE if E.plan(s, s)["jac"] == 0 and E.plan(s, s)["live"] == 1 and s > 1)


def test_blocksparse_table():
    assert sorted(E.BLOCKSPARSE_CASES) == [(1536, 20), (1590, 100)] and E.BLOCKSPARSE_TWIN == (1535, 20)
    assert [E.plan(s, K)["b"] for s, K in E.BLOCKSPARSE_CASES] == [48, 128]
    assert all(E.plan(s, K)["bs"] for s, K in E.BLOCKSPARSE_CASES) and not E.plan(*E.BLOCKSPARSE_TWIN)["bs"]
    assert E.plan(*E.BLOCKSPARSE_TWIN)["b"] == 48 and 1590 % 64 == 54


def test_stride_special_and_tol_tables():
    """the three routes each take both stride pairs; an odd ldg - s, an ldv == s and an ldv != s are among them"""
    assert sorted(E.STRIDES) == [(1, 3), (2, 0)]
    assert sorted(E.STRIDE_CASES) == sorted([("default", 48, 48), ("default", 640, 150), ("default", 301, 20), ("bs", 1536, 20)])
    plans = {(kind, s, K): E.plan(s, K) for kind, s, K in E.STRIDE_CASES}
    assert plans[("default", 48, 48)]["dense"]
    assert plans[("default", 640, 150)]["rot"] and not plans[("default", 301, 20)]["rot"]
    assert not plans[("default", 640, 150)]["bs"] and plans[("bs", 1536, 20)]["bs"]
    assert sorted(E.SPECIAL_CASES) == [(300, 20), (416, 200), (640, 150), (900, 330)]
    assert sorted(E.SPECIAL_KINDS) == ["cluster", "rank", "scaled-down", "scaled-up"]
    assert E.rank_of(300, 20) == 40 < E.plan(300, 20)["b"]              # the filtered block is rank-deficient
    assert all(E.rank_of(s, K) == K + 10 for s, K in E.SPECIAL_CASES if (s, K) != (300, 20))
    assert sorted(E.TOL_CASES) == [("bs", 1536, 20), ("default", 640, 150)] and sorted(E.TOLS) == [1e-8, 1e-6]
    assert E.REFUSAL_CASE == (300, 20)


def test_spectra():
    import numpy as np
    rng = np.random.default_rng(0)
    lam = E.spectrum("default", 300, None, rng)
    assert lam[0] == lam[1] == 1.0 and lam[2] == 1.0 - 1e-10 and (np.diff(lam) <= 0).all() and lam[3] < 0.97
    lam = E.spectrum("rank", 300, 40, rng)
    assert np.count_nonzero(lam) == 40 and lam[39] == 0.2 and lam[0] == 1.0
    K = 20
    lam = E.spectrum("cluster", 300, K, rng)
    assert (np.diff(lam) <= 0).all() and len(set(lam[K - 3:K + 2])) == 1 and lam[K - 4] > lam[K - 1] > lam[K + 2] >= 0.2
    for s in (1, 2, 3):
        assert len(E.spectrum("default", s, None, rng)) == s


def test_ring_gram_is_sparse_symmetric_with_top_eigenvalue_one():
    import numpy as np
    G = E.ring_gram(128, np.random.default_rng(1))
    assert (G == G.T).all() and np.count_nonzero(G) <= 128 * 11
    w = np.linalg.eigvalsh(G)
    assert abs(w[-1] - 1.0) < 1e-12 and w[0] > -1e-12
