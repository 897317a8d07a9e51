"""Helpers of the eigensolver edge tests (test_eig_case_table.py on the CPU, test_gpu_eig_edges.py on the GPU).

* plan(): a pure-Python restatement of what csrc/eig.hip decides from (s, K) alone with the default tuning -- eig_block_size,
  eig_use_dense, jacobi_plan, refine_route, eig_try_blocksparse -- and of rot.hip's rot_applicable for the aligned buffers the
  solver carves.  plan_ints() is the plan in the layout of flgp_dev_eig_plan; features() names the paths a plan takes.
* the case tables the GPU tests run.  test_eig_case_table.py asserts with plan() that they reach every path of the list
  required_features(), row by row.
* spectra and matrices: the project's spectrum (three copies of 1, a uniform tail), a rank-deficient one, a cluster straddling
  position K, and the Gram matrix A^T A of a sparse ring graph with its anchors permuted (the block-sparse route).
* Placement: G column-major with leading dimension ldg in a buffer of NaN, the results and the workspace in buffers of canaries.
"""
from __future__ import annotations

import functools

import numpy as np

GUARD_PCT, GUARD_MIN = 25, 24          # csrc/eig.hip: eig_guard_pct and the floor of eig_block_size
BS_MIN_S = 1536                        # eig_bs_min_s
LDS_BUDGET = 150 * 1024                # jacobi_plan
CANARY_BITS = 0x7FF8C0DEFACE0BAD       # a quiet NaN with a payload: compared bit for bit, and poison if it is ever read
CANARY_TAIL_BYTES = 4096               # behind the workspace
KERNEL = {32: "block32", 16: "block16", -1: "streamed", 0: "scalar"}


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------- the decisions, restated
def jacobi_plan(b):
    """jacobi_plan: the kernel (nloc), the block-column width, the block columns after padding, the live ones"""
    def out(nloc, w, floor2=False):
        live = ceil_div(b, w)
        nbc = live + (live & 1)
        if floor2:
            nbc = max(nbc, 2)
        return dict(nloc=nloc, w=w, nbc=nbc, live=live)
    if b % 16 == 0 and b >= 32:
        for nloc in (32, 16):
            if 8 * (nloc * (b + 2) + 6 * nloc * nloc) <= LDS_BUDGET:
                return out(nloc, nloc // 2)
    if b > 1024:
        return out(-1, 16)
    w = LDS_BUDGET // (8 * 4 * (b + 16))
    pw = 1
    while pw * 2 <= w and pw < 32:
        pw *= 2
    return out(0, pw, floor2=True)


def block_size(s, K):
    """eig_block_size"""
    guard = max(K * GUARD_PCT // 100, GUARD_MIN)
    return min((K + guard + 15) // 16 * 16, s)


def refine_route(b, K):
    """refine_route: 0 = a full jacobi_eig, 1 = small_sym_eig_kernel<64>, 2 = the block Jacobi on the guard block"""
    g = b - K
    if g < 2 or 2 * g * g > b * b:
        return 0
    return 1 if g <= 64 else 2


def plan(s, K):
    assert 1 <= K <= s
    bt = block_size(s, K)
    dense = K >= s or s <= 256 or 2 * bt >= s
    b = s if dense else bt
    jp = jacobi_plan(b)
    route = 0 if dense else refine_route(b, K)
    sub = jacobi_plan(b - K) if route == 2 else None
    return dict(s=s, K=K, dense=dense, b=b, jac=jp["nloc"], w=jp["w"], nbc=jp["nbc"], live=jp["live"], refine=route, sub=sub,
                g=b - K, bs=(not dense) and BS_MIN_S <= s <= 65536,
                rot=(not dense) and 64 <= b <= 256 and b % 64 == 0 and s % 2 == 0)


def plan_ints(p):
    """the eight ints of flgp_dev_eig_plan"""
    return [int(p["dense"]), p["b"], p["jac"], p["nbc"], p["refine"], p["sub"]["nloc"] if p["sub"] else 0, p["g"], int(p["bs"])]


def _kernel_features(where, b, jp):
    kern = KERNEL[jp["nloc"]]
    f = {(where, kern)}
    if jp["nbc"] > jp["live"]:
        f.add((where, kern, "phantom block column"))
    if kern == "block32":
        if jp["nbc"] == 2:
            f.add((where, kern, "one workgroup, one round"))
        if jacobi_plan(b + 16)["nloc"] != 32:
            f.add((where, kern, "last b"))
    if kern == "block16":
        f.add((where, kern, "register-staged load" if b <= 512 else "looped load"))
        if jacobi_plan(b - 16)["nloc"] == 32:
            f.add((where, kern, "first b"))
        if b == 512:
            f.add((where, kern, "last register-staged load"))
        if b == 528:
            f.add((where, kern, "first looped load"))
        if jacobi_plan(b + 16)["nloc"] != 16:
            f.add((where, kern, "last b"))
    if kern == "streamed":
        f.add((where, kern, "ragged rows and block column" if b % 16 else "whole block columns"))
        if b % 16 == 0 and jacobi_plan(b - 16)["nloc"] == 16:
            f.add((where, kern, "first b"))
    if kern == "scalar":
        if jp["live"] == 1:
            f.add((where, kern, "one live block column"))
        if b % 2:
            f.add((where, kern, "odd live columns"))
        if b == 1:
            f.add((where, kern, "one column"))
        if jp["w"] <= 4:
            f.add((where, kern, "narrow panel"))
    return f


def features(p):
    """the paths a plan takes, as tuples"""
    where = "dense" if p["dense"] else "truncated"
    f = _kernel_features(where, p["b"], dict(nloc=p["jac"], w=p["w"], nbc=p["nbc"], live=p["live"]))
    if p["dense"]:
        if p["K"] < p["s"] and p["s"] > 256:
            f.add(("dense", "forced by 2b >= s"))
        return f
    f.add(("truncated", "b", p["b"]))
    if p["refine"] == 0:
        f.add(("refine", "full Jacobi"))
    elif p["refine"] == 1:
        f.add(("refine", "small64"))
        if p["g"] == GUARD_MIN:
            f.add(("refine", "small64", "minimum guard"))
        if p["g"] == 64:
            f.add(("refine", "small64", "last g"))
    else:
        f |= _kernel_features("sub-Jacobi", p["g"], p["sub"])
        if p["g"] == 65:
            f.add(("sub-Jacobi", "first g"))
    if p["rot"]:
        f.add(("products", "rot"))
    elif 64 <= p["b"] <= 256 and p["b"] % 64 == 0:
        f.add(("products", "gemm", "odd s"))
    else:
        f.add(("products", "gemm", "b"))
    if p["bs"]:
        f.add(("block-sparse", "tried"))
        if p["s"] == BS_MIN_S:
            f.add(("block-sparse", "first s"))
        if p["s"] % 64:
            f.add(("block-sparse", "ragged tile"))
    elif p["s"] == BS_MIN_S - 1:
        f.add(("block-sparse", "last s below"))
    return f


def required_features():
    need = set()
    # the truncated solve: every block width of the table, the three kernels at their boundaries
    need |= {("truncated", "b", b) for b in (32, 48, 80, 192, 304, 320, 400, 416, 512, 1088, 1104)}
    need |= {("truncated", "block32"), ("truncated", "block32", "one workgroup, one round"),
             ("truncated", "block32", "phantom block column"), ("truncated", "block32", "last b"),
             ("truncated", "block16"), ("truncated", "block16", "first b"), ("truncated", "block16", "register-staged load"),
             ("truncated", "block16", "last register-staged load"), ("truncated", "block16", "looped load"),
             ("truncated", "block16", "last b"), ("truncated", "streamed"), ("truncated", "streamed", "first b")}
    # the late refinement
    need |= {("refine", "full Jacobi"), ("refine", "small64"), ("refine", "small64", "minimum guard"),
             ("refine", "small64", "last g"), ("sub-Jacobi", "first g"), ("sub-Jacobi", "scalar"), ("sub-Jacobi", "block32"),
             ("sub-Jacobi", "block32", "phantom block column")}
    need |= {("products", "rot"), ("products", "gemm", "odd s"), ("products", "gemm", "b")}
    # the dense route
    need |= {("dense", "scalar"), ("dense", "scalar", "one live block column"), ("dense", "scalar", "odd live columns"),
             ("dense", "scalar", "one column"), ("dense", "scalar", "narrow panel"),
             ("dense", "block32"), ("dense", "block32", "one workgroup, one round"), ("dense", "block32", "phantom block column"),
             ("dense", "block32", "last b"), ("dense", "block16"), ("dense", "block16", "first b"),
             ("dense", "block16", "last register-staged load"), ("dense", "block16", "first looped load"),
             ("dense", "block16", "last b"), ("dense", "streamed"), ("dense", "streamed", "ragged rows and block column"),
             ("dense", "streamed", "whole block columns"), ("dense", "streamed", "first b"), ("dense", "forced by 2b >= s")}
    need |= {("block-sparse", "tried"), ("block-sparse", "first s"), ("block-sparse", "ragged tile"),
             ("block-sparse", "last s below")}
    return need


# ------------------------------------------------------------------------------------------------- the tables
TRUNCATED_CASES = [(257, 1), (258, 8), (300, 20), (301, 20), (420, 56), (640, 150), (641, 150), (700, 240), (700, 255),
                   (900, 320), (900, 330), (1100, 400), (2300, 870), (2300, 880)]
DENSE_CASES = [(s, s) for s in (1, 2, 3, 16, 31, 32, 48, 400, 416, 512, 528, 1023, 1025, 1088, 1104)] + [(416, 200)]
BLOCKSPARSE_CASES = [(1536, 20), (1590, 100)]
BLOCKSPARSE_TWIN = (1535, 20)          # one below the switch: the same kind of matrix through the dense-G products
STRIDES = [(1, 3), (2, 0)]             # (ldg - s, ldv - s): ldg = s + 1 puts every other column of G off 16-byte alignment
STRIDE_CASES = [("default", 48, 48), ("default", 640, 150), ("default", 301, 20), ("bs", 1536, 20)]
SPECIAL_CASES = [(300, 20), (640, 150), (900, 330), (416, 200)]     # also solved with the spectra of SPECIAL_KINDS
SPECIAL_KINDS = ["rank", "cluster", "scaled-down", "scaled-up"]
TOL_CASES = [("default", 640, 150), ("bs", 1536, 20)]
TOLS = [1e-6, 1e-8]
REFUSAL_CASE = (300, 20)
# Seeds: the default is s, so that cases of one s share a matrix and its LAPACK decomposition.  An entry here replaces it for a
# case that otherwise converges before its third outer iteration (see test_gpu_eig_edges.py).
SEEDS = {}


def all_cases():
    return TRUNCATED_CASES + DENSE_CASES + BLOCKSPARSE_CASES + [BLOCKSPARSE_TWIN]


def rank_of(s, K):
    """the rank of the rank-deficient matrix of a special case: below b at (300, 20), K + 10 elsewhere"""
    return 40 if (s, K) == (300, 20) else K + 10


# ------------------------------------------------------------------------------------------------- matrices
def _rotate(lam, rng):
    s = len(lam)
    Q, _ = np.linalg.qr(rng.normal(size=(s, s)))
    G = (Q * lam) @ Q.T
    return 0.5 * (G + G.T)


def default_spectrum(s, rng):
    """the project's: three copies of 1 (the third 1e-10 below) and a sorted uniform tail below 0.97"""
    lam = np.concatenate([[1.0, 1.0, 1.0 - 1e-10], np.sort(rng.uniform(0.0, 0.97, max(s - 3, 0)))[::-1]])
    return lam[:s]


def spectrum(kind, s, param, rng):
    if kind == "default":
        return default_spectrum(s, rng)
    if kind == "rank":              # param = the rank: eigenvalues from 1 down to 0.2, exact zeros behind
        return np.concatenate([np.linspace(1.0, 0.2, param), np.zeros(s - param)])
    if kind == "cluster":           # param = K: positions K-2 .. K+2 (counted from 1) hold one value
        lam = default_spectrum(s, rng)
        lam[param - 3:param + 2] = lam[param - 1]
        return lam
    raise ValueError(kind)


def ring_gram(s, rng, n_per=20, r=6):
    """G = A^T A of a sparse n x s matrix A: r consecutive columns (mod s) per row with random positive weights, rows
    normalised to sum 1, columns scaled by 1 / sqrt(column sum), anchors permuted at random"""
    import scipy.sparse as sp
    n = n_per * s
    start = rng.integers(0, s, size=n)
    cols = (start[:, None] + np.arange(r)[None, :]) % s
    vals = rng.uniform(0.1, 1.0, size=(n, r))
    vals /= vals.sum(1, keepdims=True)
    A = sp.csr_matrix((vals.ravel(), (np.repeat(np.arange(n), r), cols.ravel())), shape=(n, s))
    csum = np.asarray(A.sum(0)).ravel()
    assert (csum > 0).all()
    A = A @ sp.diags(1.0 / np.sqrt(csum))
    A = A[:, rng.permutation(s)]
    G = np.asarray((A.T @ A).todense())
    return 0.5 * (G + G.T)


@functools.lru_cache(maxsize=None)
def problem(kind, s, param=None, seed=None):
    """(G, eigenvalues descending, eigenvectors in that order) -- the reference is LAPACK's (numpy.linalg.eigh) on the same
    float64 G, computed once per matrix.  The arrays are shared: nobody writes to them."""
    rng = np.random.default_rng(s if seed is None else seed)
    G = ring_gram(s, rng) if kind == "bs" else _rotate(spectrum(kind, s, param, rng), rng)
    w, V = np.linalg.eigh(G)
    w, V = w[::-1].copy(), V[:, ::-1].copy()
    for a in (G, w, V):
        a.setflags(write=False)
    return G, w, V


def special_problem(kind, s, K):
    """(G, w, V, scale) of a SPECIAL_KINDS case.  A power of two scales G, its eigenvalues and every operation of LAPACK
    exactly (nothing is near the ends of the exponent range), so the scaled cases reuse the default decomposition."""
    if kind == "rank":
        return problem("rank", s, rank_of(s, K)) + (1.0,)
    if kind == "cluster":
        return problem("cluster", s, K) + (1.0,)
    scale = {"scaled-down": 2.0 ** -40, "scaled-up": 2.0 ** 40}[kind]
    G, w, V = problem("default", s, None, SEEDS.get((s, K)))
    return G * scale, w * scale, V, scale


# ------------------------------------------------------------------------------------------------- placement
class Placement:
    """One call's device buffers.  G (s x s, symmetric) lies column-major with leading dimension ldg in a buffer of NaN;
    d_values has K + 8 slots, dV (K + 1) * ldv, the workspace work_bytes and CANARY_TAIL_BYTES more -- every slot a canary."""

    def __init__(self, G, K, ldg, ldv, work_bytes, device="cuda"):
        import torch
        s = G.shape[0]
        assert ldg >= s and ldv >= s and work_bytes % 8 == 0
        self.s, self.K, self.ldg, self.ldv, self.work_bytes = s, K, ldg, ldv, work_bytes
        host = np.full((s, ldg), np.nan)
        host[:, :s] = G.T                                   # column j of G at j * ldg
        self.G = torch.from_numpy(host.ravel()).to(device)
        self.values = self._canaries(K + 8, device)
        self.V = self._canaries((K + 1) * ldv, device)
        self.work = self._canaries(work_bytes // 8 + CANARY_TAIL_BYTES // 8, device)
        assert all(t.data_ptr() % 16 == 0 for t in (self.G, self.values, self.V, self.work))

    @staticmethod
    def _canaries(n, device):
        import torch
        return torch.full((n,), CANARY_BITS, dtype=torch.int64, device=device)

    def read_values(self):
        return self.values.cpu().numpy().view(np.float64)[:self.K].copy()

    def read_vectors(self):
        """s x K"""
        v = self.V.cpu().numpy().view(np.float64)[:self.K * self.ldv].reshape(self.K, self.ldv)
        return np.ascontiguousarray(v[:, :self.s].T)

    def damage(self):
        """what is wrong outside and inside the results: a list of messages (empty: all well)"""
        out = []
        vals = self.values.cpu().numpy()
        if not (vals[self.K:] == CANARY_BITS).all():
            out.append("a store behind the K values")
        if not np.isfinite(vals[:self.K].view(np.float64)).all():
            out.append("a value that is not finite (or was never written)")
        V = self.V.cpu().numpy().reshape(self.K + 1, self.ldv)
        if not (V[:self.K, self.s:] == CANARY_BITS).all():
            out.append("a store into the padding rows of V (ldv)")
        if not (V[self.K] == CANARY_BITS).all():
            out.append("a store behind the K columns of V")
        if not np.isfinite(V[:self.K, :self.s].view(np.float64)).all():
            out.append("an element of V that is not finite (or was never written)")
        tail = self.work[self.work_bytes // 8:].cpu().numpy()
        if not (tail == CANARY_BITS).all():
            out.append("a store behind the workspace size flgp_dev_eig_workspace reports")
        return out
