"""Host-side mirror of FLGP's R-visible interface for the heat-kernel covariance path.

R is not available in this image, so the layer FLGP users see (``R/RcppExports.R`` +
``R/Fit.R:760-770``) is mirrored here in Python with the same function names, argument
names, defaults and error behaviour, each call going straight through the C ABI of
``libflgp_hip.so`` (``include/flgp_hip.h``) -- the same entry points the R ``.Call`` shim
binds (``flgp_amd/csrc/rshim/flgp_rcall.c``).  Nothing here computes: numpy
arrays are R's column-major matrices, scipy CSR matrices stand in for ``Matrix::dgRMatrix``.

Anchors: ``subsample_cpp`` (reference src/Utils.cpp:32-68) is R's ``stats::kmeans`` /
``ClusterR`` / ``sample`` and is outside the accelerated path.  Functions that subsample
inside the reference take the anchors through the extra keyword ``U`` (s x d, or s x (d+1)
with cluster sizes in the last column); ``subsample="random"`` is also provided (seeded
numpy RNG in place of R's).
"""
from __future__ import annotations

from dataclasses import dataclass

import ctypes

import numpy as np

from . import _lib
from ._lib import FlgpError, check  # noqa: F401

_DEFAULT_MODELS_CPP = dict(subsample="kmeans", kernel="lae", gl="rw", root=False)          # src/Spectrum.h:53-59
_DEFAULT_MODELS_R = dict(subsample="kmeans", kernel="lae", gl="cluster-normalized", root=True)  # R/Fit.R:761-764


def _f64(a, name="matrix"):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        a = a.reshape(-1, 1)
    if a.ndim != 2:
        raise ValueError(f"{name} must be a matrix")
    return np.asfortranarray(a)


def _ptr(a):
    return None if a is None else a.ctypes.data


def _b(s):
    return str(s).encode("utf-8")


@dataclass
class EigenPair:
    """``EigenPair`` (reference src/Spectrum.h:117-124): eigenvalues of W (sigma^2, or sigma
    when root), NOT of the Laplacian; ``vectors`` is n x K = U sqrt(n)."""
    values: np.ndarray
    vectors: np.ndarray


def _csr(n, s, r, p, j, x):
    import scipy.sparse as sp
    return sp.csr_matrix((x, j, p), shape=(n, s))


def _csr_parts(Z, what="Z"):
    import scipy.sparse as sp
    Z = sp.csr_matrix(Z)
    n, s = Z.shape
    nnz_row = np.diff(Z.indptr)
    if n == 0 or not np.all(nnz_row == nnz_row[0]):
        raise ValueError(f"{what} must store the same number of entries in every row (k-NN sparsity)")
    Z.sort_indices()
    r = int(nnz_row[0])
    return n, s, r, np.ascontiguousarray(Z.indices, dtype=np.int32), np.ascontiguousarray(Z.data, dtype=np.float64)


def KNN_cpp(X, U, r=3, distance="Euclidean", output=False, batch=100):
    """KNN_cpp (src/Utils.cpp:102-192, src/Utils.h:60-62).  Returns ``{"ind_knn": n x r int32
    (0-based)}`` plus ``"distances_sp"`` (CSR n x s) when ``output``.  ``batch`` is accepted
    and ignored: it has no numerical effect in the reference either."""
    del batch
    X = _f64(X, "X"); U = _f64(U, "U")
    n, d = X.shape; s = U.shape[0]
    if U.shape[1] != d:
        raise ValueError("X and U must have the same number of columns")
    ind = np.zeros((n, r), dtype=np.int32, order="F")
    dist = np.zeros((n, r), dtype=np.float64, order="F") if output else None
    check(_lib.lib().flgp_knn(_ptr(X), n, d, _ptr(U), s, int(r), _b(distance), _ptr(ind), _ptr(dist)))
    res = {"ind_knn": ind}
    if output:
        import scipy.sparse as sp
        order = np.argsort(ind, axis=1, kind="stable")
        j = np.take_along_axis(ind, order, axis=1)
        x = np.take_along_axis(dist, order, axis=1)
        res["distances_sp"] = sp.csr_matrix((x.ravel(), j.ravel(), np.arange(0, n * r + 1, r)), shape=(n, s))
    return res


def v_to_z_cpp(v):
    """v_to_z_cpp (src/lae.cpp:137-153)."""
    v = np.ascontiguousarray(v, dtype=np.float64).ravel()
    z = np.zeros_like(v)
    check(_lib.lib().flgp_v_to_z(_ptr(v), v.size, _ptr(z)))
    return z.reshape(1, -1)


def local_anchor_embedding_cpp(x, U):
    """local_anchor_embedding_cpp (src/lae.cpp:76-133): x length d, U r x d -> 1 x r."""
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    U = _f64(U, "U")
    r, d = U.shape
    if x.size != d:
        raise ValueError("x and U must have the same dimension")
    z = np.zeros(r)
    check(_lib.lib().flgp_local_anchor_embedding(_ptr(x), d, _ptr(U), r, _ptr(z)))
    return z.reshape(1, -1)


def LAE_cpp(X, U, r=3):
    """LAE_cpp (src/lae.cpp:48-70) -> CSR n x s with exactly r stored entries per row."""
    X = _f64(X, "X"); U = _f64(U, "U")
    n, d = X.shape; s = U.shape[0]
    if U.shape[1] != d:
        raise ValueError("X and U must have the same number of columns")
    p = np.zeros(n + 1, dtype=np.int32); j = np.zeros(n * r, dtype=np.int32); x = np.zeros(n * r)
    check(_lib.lib().flgp_lae(_ptr(X), n, d, _ptr(U), s, int(r), _ptr(p), _ptr(j), _ptr(x)))
    return _csr(n, s, r, p, j, x)


def cross_similarity_lae_cpp(X, U, r=3, gl="rw"):
    """cross_similarity_lae_cpp (src/Spectrum.cpp:101-117, defaults src/Spectrum.h:88-92)."""
    X = _f64(X, "X"); U = _f64(U, "U")
    n, d = X.shape; s, ucols = U.shape
    p = np.zeros(n + 1, dtype=np.int32); j = np.zeros(n * r, dtype=np.int32); x = np.zeros(n * r)
    check(_lib.lib().flgp_cross_similarity_lae(_ptr(X), n, d, _ptr(U), s, ucols, int(r), _b(gl), _ptr(p), _ptr(j), _ptr(x)))
    return _csr(n, s, r, p, j, x)


def cross_similarity_se_cpp(X, U, r, gl, epsilon):
    """cross_similarity_se_cpp (src/Spectrum.cpp:120-142)."""
    X = _f64(X, "X"); U = _f64(U, "U")
    n, d = X.shape; s, ucols = U.shape
    p = np.zeros(n + 1, dtype=np.int32); j = np.zeros(n * r, dtype=np.int32); x = np.zeros(n * r)
    check(_lib.lib().flgp_cross_similarity_se(_ptr(X), n, d, _ptr(U), s, ucols, int(r), _b(gl), float(epsilon),
                                              _ptr(p), _ptr(j), _ptr(x)))
    return _csr(n, s, r, p, j, x)


def graphLaplacian_cpp(Z, gl, num_class=None):
    """graphLaplacian_cpp (src/Utils.cpp:195-212).  The reference normalises Z in place; this
    returns the normalised copy."""
    n, s, r, j, x = _csr_parts(Z)
    x = x.copy()
    nc = None if num_class is None else np.ascontiguousarray(num_class, dtype=np.float64)
    check(_lib.lib().flgp_graph_laplacian(_ptr(j), _ptr(x), n, s, r, _b(gl), _ptr(nc)))
    return _csr(n, s, r, np.arange(0, n * r + 1, r, dtype=np.int32), j, x)


def spectrum_from_Z_cpp(Z, K, root=False):
    """spectrum_from_Z_cpp (src/Spectrum.cpp:146-161) incl. truncated_SVD_cpp (src/TruncatedSVD.cpp:9-34)."""
    n, s, r, j, x = _csr_parts(Z)
    Kk = s if K < 0 else int(K)
    values = np.zeros(Kk); vectors = np.zeros((n, Kk), order="F")
    check(_lib.lib().flgp_spectrum_from_Z(_ptr(j), _ptr(x), n, s, r, int(K), int(bool(root)), _ptr(values), _ptr(vectors)))
    return EigenPair(values, vectors)


def HK_from_spectrum_cpp(eigenpair, K, t, idx0, idx1):
    """HK_from_spectrum_cpp (src/Spectrum.cpp:83-94); idx0 / idx1 are 0-based row indices."""
    vec = _f64(eigenpair.vectors, "vectors")
    vals = np.ascontiguousarray(eigenpair.values, dtype=np.float64)
    n = vec.shape[0]
    if K > vec.shape[1] or K > vals.size:
        raise ValueError("K exceeds the number of stored eigenpairs")
    idx0 = np.ascontiguousarray(idx0, dtype=np.int32); idx1 = np.ascontiguousarray(idx1, dtype=np.int32)
    H = np.zeros((idx0.size, idx1.size), order="F")
    check(_lib.lib().flgp_hk_from_spectrum(_ptr(vals), _ptr(vec), n, int(K), float(t), _ptr(idx0), idx0.size,
                                           _ptr(idx1), idx1.size, _ptr(H)))
    return H


def marginal_log_likelihood_logit_la_cpp(C, Y, N, tol=1e-5, max_iter=100, return_iters=False):
    """marginal_log_likelihood_logit_la_cpp (src/train.cpp:716-760; defaults src/train.h:35-36): the Laplace-approximate
    log marginal likelihood of the binomial logit GP with covariance C (m x m), Y successes of N trials per row.  Newton's
    loop and its Cholesky factorisations run on the device.  ``return_iters``: also return the Newton iterations run."""
    C = _f64(C, "C")
    m = C.shape[0]
    if C.shape != (m, m):
        raise ValueError("C must be square")
    Y = np.ascontiguousarray(np.asarray(Y, dtype=np.float64).reshape(-1))
    N = np.ascontiguousarray(np.broadcast_to(np.asarray(N, dtype=np.float64), (m,)))
    if Y.size != m:
        raise ValueError("Y must have one entry per row of C")
    amll = ctypes.c_double(); it = ctypes.c_int()
    check(_lib.lib().flgp_logit_la_marginal_likelihood(_ptr(C), m, _ptr(Y), _ptr(N), float(tol), int(max_iter),
                                                       ctypes.byref(amll), ctypes.byref(it)))
    return (amll.value, it.value) if return_iters else amll.value


def multi_train_split(Y):
    """multi_train_split (src/MultiClassification.cpp:14-26): one 0/1 column per class 0 .. max(Y)."""
    Y = np.asarray(Y).reshape(-1)
    J = int(Y.max()) + 1
    return (Y[:, None] == np.arange(J)[None, :]).astype(np.float64)


def _seed(seed):
    """A chain's seed: the caller's, or one drawn from numpy's default generator.  R passes one drawn from its own RNG, so
    that ``set.seed`` still reproduces a fit ("Polya-Gamma prediction")."""
    if seed is None:
        return int(np.random.default_rng().integers(0, 2**63))
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def pgdraw(b, c, seed=None):
    """pgdraw(b, c) (BayesLogit / pgdraw's contract): omega_i ~ PG(b_i, c_i), drawn on the device.  ``b`` is a positive
    integer or one per entry (None: all ones); the draws are reproducible from ``seed`` (pg.hip documents the layout)."""
    c = np.ascontiguousarray(np.asarray(c, dtype=np.float64).reshape(-1))
    bb = None if b is None else np.ascontiguousarray(np.broadcast_to(np.asarray(b, dtype=np.float64), c.shape))
    out = np.zeros(c.size)
    check(_lib.lib().flgp_pg_draw(_ptr(bb), _ptr(c), c.size, _seed(seed), _ptr(out)))
    return out


def test_pgbinary_cpp(C, Y, Cnv, N_sample=100, output_pi=False, seed=None):
    """test_pgbinary_cpp (src/Predict.cpp:11-26; defaults src/Predict.h:33-37): N_sample Gibbs sweeps of the Polya-Gamma
    logit model with covariance C (m x m), then the collapsed prediction of the rows of Cnv (m_new x m).  Returns the R
    list's keys: {"Y_pred"} and, with ``output_pi``, "pi_pred"."""
    C = _f64(C, "C")
    m = C.shape[0]
    if C.shape != (m, m):
        raise ValueError("C must be square")
    Cnv = _f64(Cnv, "Cnv")
    if Cnv.shape[1] != m:
        raise ValueError("Cnv must have one column per row of C")
    Y = np.ascontiguousarray(np.asarray(Y, dtype=np.float64).reshape(-1))
    if Y.size != m:
        raise ValueError("Y must have one entry per row of C")
    mnew = Cnv.shape[0]
    pi = np.zeros(mnew); y = np.zeros(mnew)
    check(_lib.lib().flgp_pg_logit_predict(_ptr(C), m, _ptr(Y), _ptr(Cnv), mnew, int(N_sample), _seed(seed), _ptr(pi), _ptr(y),
                                           None, None))
    return {"Y_pred": y, "pi_pred": pi} if output_pi else {"Y_pred": y}


def _pg_logit_predict_state(C, Y, Cnv, N_sample, seed):
    """test_pgbinary_cpp with the chain's final omega and f as well: (pi_pred, Y_pred, omega, f)."""
    C = _f64(C, "C"); Cnv = _f64(Cnv, "Cnv")
    m = C.shape[0]
    Y = np.ascontiguousarray(np.asarray(Y, dtype=np.float64).reshape(-1))
    pi = np.zeros(Cnv.shape[0]); y = np.zeros(Cnv.shape[0]); om = np.zeros(m); f = np.zeros(m)
    check(_lib.lib().flgp_pg_logit_predict(_ptr(C), m, _ptr(Y), _ptr(Cnv), Cnv.shape[0], int(N_sample), _seed(seed), _ptr(pi),
                                           _ptr(y), _ptr(om), _ptr(f)))
    return pi, y, om, f


def negative_log_likelihood(mean, cov, target, type, n_samples=100, seed=None, return_like=False):
    """negative_log_likelihood (src/Utils.cpp:302-318), on the device: the score of a ``posterior`` list.  ``type`` is
    "regression", "binary" (``nll_classification``) or "multinomial" (``target`` holds class labels 0 .. J-1, ``mean`` and
    ``cov`` are n x J).  The classification types average the logistic likelihood over ``n_samples`` normals per row (the
    reference fixes 100), reproducible from ``seed`` (nll.hip documents the layout).  ``return_like``: also the per-row
    likelihoods (n, or n x J), for "regression" the per-row terms."""
    target = np.ascontiguousarray(np.asarray(target, dtype=np.float64).reshape(-1))
    n = target.size
    mean = np.asarray(mean, dtype=np.float64); cov = np.asarray(cov, dtype=np.float64)
    if type == "multinomial":
        if mean.ndim != 2 or mean.shape[0] != n or cov.shape != mean.shape:
            raise ValueError("mean and cov must be n x J matrices with one row per entry of target")
        mean = np.asfortranarray(mean); cov = np.asfortranarray(cov)
        J = mean.shape[1]
    else:
        if mean.size != n or cov.size != n:
            raise ValueError("mean and cov must be vectors with one entry per entry of target")
        mean = np.ascontiguousarray(mean.reshape(-1)); cov = np.ascontiguousarray(cov.reshape(-1))
        J = 1
    nll = ctypes.c_double()
    like = np.zeros(mean.shape, order="F") if return_like else None
    check(_lib.lib().flgp_negative_log_likelihood(_ptr(mean), _ptr(cov), _ptr(target), n, J, _b(type), int(n_samples), _seed(seed),
                                                  ctypes.byref(nll), _ptr(like)))
    return (nll.value, like) if return_like else nll.value


def nll_classification(mean, cov, target, n_samples=100, seed=None, return_like=False):
    """nll_classification (src/Utils.cpp:321-336; default src/Utils.h): the "binary" route of negative_log_likelihood."""
    return negative_log_likelihood(mean, cov, target, "binary", n_samples, seed, return_like)


class ResidentEigenPair:
    """An ``EigenPair`` that stays in HBM (include/flgp_hip.h, "device-resident EigenPair"): what the training
    loop needs, since it calls ``HK_from_spectrum_cpp`` with the same pair and a new ``t`` on every objective
    evaluation (reference src/train.cpp:17,30,363,471).  On the R side the handle is an external pointer."""

    def __init__(self, handle):
        self._h = handle
        n = ctypes.c_int(); K = ctypes.c_int()
        check(_lib.lib().flgp_eigenpair_dims(self._h, ctypes.byref(n), ctypes.byref(K)))
        self.n, self.K = n.value, K.value

    @classmethod
    def from_host(cls, eigenpair):
        vec = _f64(eigenpair.vectors, "vectors")
        vals = np.ascontiguousarray(eigenpair.values, dtype=np.float64)
        h = ctypes.c_void_p()
        check(_lib.lib().flgp_eigenpair_from_host(_ptr(vals), _ptr(vec), vec.shape[0], vals.size, ctypes.byref(h)))
        return cls(h)

    def HK_from_spectrum_cpp(self, K, t, idx0, idx1):
        idx0 = np.ascontiguousarray(idx0, dtype=np.int32); idx1 = np.ascontiguousarray(idx1, dtype=np.int32)
        H = np.zeros((idx0.size, idx1.size), order="F")
        check(_lib.lib().flgp_hk_from_eigenpair(self._h, int(K), float(t), _ptr(idx0), idx0.size, _ptr(idx1), idx1.size,
                                                _ptr(H)))
        return H

    def VtV(self, K, idx):
        """V^T V for V = vectors[idx, 0:K] (src/train.cpp:400)"""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        out = np.zeros((K, K), order="F")
        check(_lib.lib().flgp_eigenpair_vtv(self._h, int(K), _ptr(idx), idx.size, _ptr(out)))
        return out

    def VtY(self, K, idx, Y):
        """V^T Y (src/train.cpp:404)"""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        Y = np.asfortranarray(np.asarray(Y, dtype=np.float64).reshape(idx.size, -1))
        out = np.zeros((K, Y.shape[1]), order="F")
        check(_lib.lib().flgp_eigenpair_vty(self._h, int(K), _ptr(idx), idx.size, _ptr(Y), Y.shape[1], _ptr(out)))
        return out

    def VC(self, K, idx, C):
        """V C for a K x q matrix C (src/train.cpp:404, src/Predict.cpp:60-75)"""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        C = np.asfortranarray(np.asarray(C, dtype=np.float64).reshape(K, -1))
        out = np.zeros((idx.size, C.shape[1]), order="F")
        check(_lib.lib().flgp_eigenpair_vc(self._h, int(K), _ptr(idx), idx.size, _ptr(C), C.shape[1], _ptr(out)))
        return out

    def predict_regression_cpp(self, Y, idx0, idx1, K, pars, sigma, noisepar="same"):
        """predict_regression_cpp (src/Predict.cpp:40-75) on the resident pair: Y (m x q) goes up, Y_pred (m_new x q)
        comes down; the Woodbury / Cholesky algebra runs on the device.  ``pars = (t, noise)`` for noisepar = "same",
        ``(t, noise_1, ..., noise_m)`` for "different" (src/Predict.cpp:76-110)."""
        idx0 = np.ascontiguousarray(idx0, dtype=np.int32); idx1 = np.ascontiguousarray(idx1, dtype=np.int32)
        Y = np.asfortranarray(np.asarray(Y, dtype=np.float64).reshape(idx0.size, -1))
        out = np.zeros((idx1.size, Y.shape[1]), order="F")
        if noisepar == "different":
            nz = np.ascontiguousarray(np.asarray(pars[1:], dtype=np.float64))
            if nz.size != idx0.size:
                raise ValueError('noisepar="different" needs one noise variance per training row: pars = (t, noise_1 .. noise_m)')
            check(_lib.lib().flgp_eigenpair_predict_regression_different(self._h, int(K), _ptr(idx0), idx0.size, _ptr(idx1), idx1.size,
                                                                         _ptr(Y), Y.shape[1], float(pars[0]), _ptr(nz), float(sigma), _ptr(out)))
            return out
        if noisepar != "same":
            raise FlgpError(-3, 'predict_regression_cpp: noisepar must be "same" or "different"')
        check(_lib.lib().flgp_eigenpair_predict_regression(self._h, int(K), _ptr(idx0), idx0.size, _ptr(idx1), idx1.size, _ptr(Y),
                                                           Y.shape[1], float(pars[0]), float(pars[1]), float(sigma), _ptr(out)))
        return out

    def posterior_covariance_regression(self, idx0, idx1, K, pars, sigma):
        """posterior_covariance_regression (src/Utils.cpp:214-250): posterior variance of the rows idx1; ``pars = (t, var)``."""
        idx0 = np.ascontiguousarray(idx0, dtype=np.int32); idx1 = np.ascontiguousarray(idx1, dtype=np.int32)
        out = np.zeros(idx1.size)
        check(_lib.lib().flgp_eigenpair_posterior_variance(self._h, int(K), _ptr(idx0), idx0.size, _ptr(idx1), idx1.size,
                                                           float(pars[0]), float(pars[1]), float(sigma), _ptr(out)))
        return out

    def regression_posterior(self, Y, idx0, idx1, K, pars, sigma, noisepar="same", target=None, train=True,
                             return_posterior=True):
        """The testing step of the four ``fit_*_regression_gp_cpp`` drivers (src/Fit.cpp:70-79) in one call
        (flgp_eigenpair_regression_posterior, include/flgp_hip.h): ``predict_regression_cpp`` on the training rows and
        on the new rows and ``posterior_covariance_regression`` at ``(pars[0], pars[1])``.  ``pars`` as
        ``predict_regression_cpp``.  m <= K gives the three existing methods' bits; m > K solves in weight space (K x K
        systems, idx0 / idx1 / Y uploaded and V1 gathered once) and reads the rows from the pair in place, in one fused
        kernel per row set; there cov >= pars[1] + sigma exactly.  Returns the drivers' list shape
        ``{"Y_pred": {"train", "test"}, "posterior": {"mean", "cov"}}`` (m x q, m_new x q Fortran-ordered; "mean" is
        "test").  ``train=False`` skips the training rows ("train" is None).  With ``target`` (m_new values, q = 1) the
        result is scored on the device as ``negative_log_likelihood(mean, cov, target, "regression")`` and "nll" is
        added; ``return_posterior=False`` then brings down that one number only."""
        idx0 = np.ascontiguousarray(idx0, dtype=np.int32); idx1 = np.ascontiguousarray(idx1, dtype=np.int32)
        m, mnew = idx0.size, idx1.size
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim > 2 or (Y.ndim == 2 and Y.shape[0] != m) or (Y.ndim < 2 and Y.size != m):
            raise ValueError("Y must have one row per entry of idx0")
        Y = np.asfortranarray(Y.reshape(m, -1))
        q = Y.shape[1]
        if noisepar not in ("same", "different"):
            raise FlgpError(-3, 'regression_posterior: noisepar must be "same" or "different"')
        nz = np.ascontiguousarray(np.asarray(pars[1:], dtype=np.float64).reshape(-1))
        if noisepar == "different" and nz.size != m:
            raise ValueError('noisepar="different" needs one noise variance per training row: pars = (t, noise_1 .. noise_m)')
        if noisepar == "same":
            nz = nz[:1].copy()
        if target is None and not return_posterior:
            raise ValueError("return_posterior=False needs a target to score")
        nll = None
        if target is not None:
            target = np.ascontiguousarray(np.asarray(target, dtype=np.float64).reshape(-1))
            if target.size != mnew:
                raise ValueError("target must have one entry per row of idx1")
            nll = ctypes.c_double()
        tr = te = cov = None
        if return_posterior:
            tr = np.zeros((m, q), order="F") if train else None
            te = np.zeros((mnew, q), order="F"); cov = np.zeros(mnew)
        check(_lib.lib().flgp_eigenpair_regression_posterior(self._h, int(K), _ptr(idx0), m, _ptr(idx1), mnew, _ptr(Y), q,
                                                             float(pars[0]), _ptr(nz), nz.size, float(sigma), _ptr(tr), _ptr(te),
                                                             _ptr(cov), _ptr(target), ctypes.addressof(nll) if nll is not None else None))
        out = {}
        if return_posterior:
            out["Y_pred"] = {"train": tr, "test": te}
            out["posterior"] = {"mean": te, "cov": cov}
        if nll is not None:
            out["nll"] = nll.value
        return out

    def marginal_log_likelihood_logit_la(self, K, t, idx, Y, N=None, sigma=1e-3, tol=1e-5, max_iter=100, return_iters=False):
        """The objective of the logit drivers' hyper-parameter search (negative_marginal_likelihood_logit_cpp,
        src/train.cpp:28-34, negated back): ``marginal_log_likelihood_logit_la_cpp(HK(idx, idx) + sigma I, Y, N)`` with C
        built on the device from the resident V; only the scalar comes back.  N defaults to one trial per row (what the
        drivers pass, src/Fit.cpp:553 and src/MultiClassification.cpp:36); sigma's default is the R wrappers' (R/Fit.R)."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        m = idx.size
        Y = np.ascontiguousarray(np.asarray(Y, dtype=np.float64).reshape(-1))
        N = np.ones(m) if N is None else np.ascontiguousarray(np.broadcast_to(np.asarray(N, dtype=np.float64), (m,)))
        if Y.size != m:
            raise ValueError("Y must have one entry per row of idx")
        amll = ctypes.c_double(); it = ctypes.c_int()
        check(_lib.lib().flgp_eigenpair_logit_marginal_likelihood(self._h, int(K), float(t), float(sigma), _ptr(idx), m, _ptr(Y),
                                                                  _ptr(N), float(tol), int(max_iter), ctypes.byref(amll),
                                                                  ctypes.byref(it)))
        return (amll.value, it.value) if return_iters else amll.value

    def posterior_distribution_classification(self, idx0, idx1, K, t, Y, sigma11, sigma22, tol=1e-5, max_iter=100):
        """posterior_distribution_classification (src/Utils.cpp:252-299; defaults src/Utils.h:80) with
        C11 = HK(idx0, idx0) + sigma11 I, C21 = HK(idx1, idx0), C22 = diag HK(idx1, idx1) + sigma22: the binary drivers
        pass sigma11 = sigma22 = sigma (src/Fit.cpp:571-583), the one-vs-rest route sigma11 = 0 (src/Utils.cpp:357-360).
        Returns {"mean", "cov"} for the rows idx1; C21 is never formed (include/flgp_hip.h)."""
        idx0 = np.ascontiguousarray(idx0, dtype=np.int32); idx1 = np.ascontiguousarray(idx1, dtype=np.int32)
        Y = np.ascontiguousarray(np.asarray(Y, dtype=np.float64).reshape(-1))
        if Y.size != idx0.size:
            raise ValueError("Y must have one entry per row of idx0")
        mean = np.zeros(idx1.size); cov = np.zeros(idx1.size)
        check(_lib.lib().flgp_eigenpair_posterior_classification(self._h, int(K), float(t), float(sigma11), float(sigma22),
                                                                 _ptr(idx0), idx0.size, _ptr(Y), _ptr(idx1), idx1.size, float(tol),
                                                                 int(max_iter), _ptr(mean), _ptr(cov)))
        return {"mean": mean, "cov": cov}

    def logit_posterior(self, idx0, idx1, K, t, Y, sigma11, sigma22, tol=1e-5, max_iter=100, return_iters=False):
        """The Laplace posterior of ``posterior_distribution_classification`` with a route of its own for more labelled
        rows than eigenpairs: m <= K gives that method's bits, m > K finds the mode in weight space (a K x K system per
        Newton iteration, no m x m matrix) and reads the rows idx1 from the pair in place, in one fused kernel
        (include/flgp_hip.h); there var >= sigma22 exactly.  sigma11, sigma22 >= 0.  Returns {"mean", "cov"} for the rows
        idx1, or ``({"mean", "cov"}, iters)`` with ``return_iters``."""
        idx0 = np.ascontiguousarray(idx0, dtype=np.int32); idx1 = np.ascontiguousarray(idx1, dtype=np.int32)
        Y = np.ascontiguousarray(np.asarray(Y, dtype=np.float64).reshape(-1))
        if Y.size != idx0.size:
            raise ValueError("Y must have one entry per row of idx0")
        mean = np.zeros(idx1.size); cov = np.zeros(idx1.size)
        it = ctypes.c_int()
        check(_lib.lib().flgp_eigenpair_logit_posterior(self._h, int(K), float(t), float(sigma11), float(sigma22), _ptr(idx0),
                                                        idx0.size, _ptr(Y), _ptr(idx1), idx1.size, float(tol), int(max_iter),
                                                        _ptr(mean), _ptr(cov), ctypes.byref(it)))
        post = {"mean": mean, "cov": cov}
        return (post, it.value) if return_iters else post

    def posterior_distribution_multiclassification(self, idx0, idx1, K, ts, Y, sigma, tol=1e-5, max_iter=100):
        """posterior_distribution_multiclassification (src/Utils.cpp:336-369): one-vs-rest over the J = max(Y) + 1 classes
        of ``multi_train_split(Y)``, class j at its own ``ts[j]``, sigma on C22 only.  Returns {"mean", "cov"}, m_new x J."""
        aug_y = multi_train_split(Y)
        J = aug_y.shape[1]
        ts = np.asarray(ts, dtype=np.float64).reshape(-1)
        if ts.size != J:
            raise ValueError(f"need one t per class: {J} classes, {ts.size} values of t")
        idx1 = np.asarray(idx1)
        mean = np.zeros((idx1.size, J), order="F"); cov = np.zeros((idx1.size, J), order="F")
        for j in range(J):
            post = self.posterior_distribution_classification(idx0, idx1, K, ts[j], aug_y[:, j], 0.0, sigma, tol, max_iter)
            mean[:, j] = post["mean"]; cov[:, j] = post["cov"]
        return {"mean": mean, "cov": cov}

    def logit_posterior_multiclass(self, idx0, idx1, K, ts, Y, sigma, sigma11=0.0, tol=1e-5, max_iter=100, max_parallel=4,
                                   return_iters=False, target=None, n_samples=100, seed=None, return_posterior=True):
        """The one-vs-rest posterior of ``posterior_distribution_multiclassification`` in one call
        (flgp_eigenpair_logit_posterior_multiclass, include/flgp_hip.h): ``Y`` holds class labels 0 .. J-1 with
        J = ``len(ts)``, class j is ``logit_posterior`` on ``Y == j`` at ``ts[j]`` with ``sigma22 = sigma`` (``sigma11``
        defaults to the reference's 0), bit for bit.  The rows, the labels and V1 go up once and, for m > K, one fused
        kernel per chunk reads the rows idx1 once for all its classes.  ``max_parallel``: for m > K the number of classes
        per chunk, whose Newton loops advance in the same launches on one stream (below 1: one class per chunk; never
        more than J or than fit the device memory); results do not depend on it.  A class without a member is allowed.
        Returns {"mean", "cov"}, m_new x J Fortran-ordered.  With ``target`` (m_new class labels naming all J classes) the result is scored on the device as
        ``negative_log_likelihood(mean, cov, target, "multinomial", n_samples, seed)`` and "nll" is added;
        ``return_posterior=False`` then brings down that one number only.  ``return_iters``: also the J iteration counts."""
        idx0 = np.ascontiguousarray(idx0, dtype=np.int32); idx1 = np.ascontiguousarray(idx1, dtype=np.int32)
        Y = np.ascontiguousarray(np.asarray(Y, dtype=np.float64).reshape(-1))
        ts = np.ascontiguousarray(np.asarray(ts, dtype=np.float64).reshape(-1))
        J = ts.size
        if Y.size != idx0.size:
            raise ValueError("Y must have one entry per row of idx0")
        if target is None and not return_posterior:
            raise ValueError("return_posterior=False needs a target to score")
        if target is not None:
            target = np.ascontiguousarray(np.asarray(target, dtype=np.float64).reshape(-1))
            if target.size != idx1.size:
                raise ValueError("target must have one entry per row of idx1")
            if target.size and np.isfinite(target).all() and int(target.max()) + 1 != J:
                raise ValueError(f"need one t per class: target names {int(target.max()) + 1} classes, {J} values of t")
        mean = cov = None
        if return_posterior:
            mean = np.zeros((idx1.size, J), order="F"); cov = np.zeros((idx1.size, J), order="F")
        its = np.zeros(max(J, 1), dtype=np.int32)
        head = (self._h, int(K), _ptr(ts), J, float(sigma11), float(sigma), _ptr(idx0), idx0.size, _ptr(Y), _ptr(idx1), idx1.size,
                float(tol), int(max_iter), int(max_parallel), _ptr(mean), _ptr(cov), _ptr(its))
        out = {}
        if target is None:
            check(_lib.lib().flgp_eigenpair_logit_posterior_multiclass(*head))
        else:
            nll = ctypes.c_double()
            check(_lib.lib().flgp_eigenpair_logit_posterior_multiclass_nll(*head, _ptr(target), int(n_samples), _seed(seed),
                                                                           ctypes.byref(nll)))
            out["nll"] = nll.value
        if return_posterior:
            out["mean"] = mean; out["cov"] = cov
        return (out, its[:J].copy()) if return_iters else out

    def logit_posterior_batch(self, idx0, idx1, K, ts, Y, col=None, sigma11=0.0, sigma22=1e-3, tol=1e-5, max_iter=100,
                              max_parallel=0, return_iters=False):
        """``logit_posterior`` for B problems in one call (flgp_eigenpair_logit_posterior_batch, include/flgp_hip.h):
        problem b is column ``col[b]`` of ``Y`` (m, or m x ncol, entries in [0, 1]; ``col`` None needs ncol == B and means
        0 .. B-1) at ``ts[b]``; the rows, K, the sigmas, tol and max_iter are shared.  Column b of the result (and its
        iteration count) is, bit for bit, ``logit_posterior`` on that column at that t, whatever else shares the call.  For
        m > K the B weight-space Newton loops advance in the same launches, ``max_parallel`` problems per chunk (0: as many
        as fit the device memory), and one fused kernel per chunk reads the rows idx1 once for all its problems; m <= K runs
        the dense route per problem.  ``logit_posterior`` is this call with B = 1 and the one-vs-rest posterior is this
        call on the m x J indicator matrix: one body in the library.  A bad ``col[b]`` or ``ts[b]`` is refused here, before
        the library is called, with the library's own text.  Returns {"mean", "cov"}, m_new x B Fortran-ordered, or ``({"mean", "cov"}, iters)``."""
        who = "logit_posterior_batch"
        idx0 = np.ascontiguousarray(idx0, dtype=np.int32); idx1 = np.ascontiguousarray(idx1, dtype=np.int32)
        m = idx0.size
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim > 2 or (Y.ndim == 2 and Y.shape[0] != m) or (Y.ndim < 2 and Y.size != m):
            raise ValueError("Y must have one row per entry of idx0")
        Y = np.asfortranarray(Y.reshape(m, -1))
        ncol = Y.shape[1]
        ts = np.ascontiguousarray(np.asarray(ts, dtype=np.float64).reshape(-1))
        B = ts.size
        if col is None and ncol != B:
            raise FlgpError(-1, f"{who}: col may be NULL only if ncol == B (ncol={ncol}, B={B})")
        cols = None if col is None else np.ascontiguousarray(np.asarray(col, dtype=np.int32).reshape(-1))
        if cols is not None and cols.size != B:
            raise ValueError("col must have one entry per value of t")
        for b in range(B):
            c = b if cols is None else int(cols[b])
            head = "problem %d (t=%g): %s: " % (b, ts[b], who)
            if not 0 <= c < ncol:
                raise FlgpError(-1, head + "col=%d is outside [0, ncol=%d)" % (c, ncol))
            if not np.isfinite(ts[b]):
                raise FlgpError(-1, head + "t must be finite")
        mean = np.zeros((idx1.size, max(B, 1)), order="F"); cov = np.zeros((idx1.size, max(B, 1)), order="F")
        its = np.zeros(max(B, 1), dtype=np.int32)
        check(_lib.lib().flgp_eigenpair_logit_posterior_batch(self._h, int(K), _ptr(idx0), m, _ptr(Y), ncol, _ptr(cols), _ptr(ts), B,
                                                              float(sigma11), float(sigma22), _ptr(idx1), idx1.size, float(tol),
                                                              int(max_iter), int(max_parallel), _ptr(mean), _ptr(cov), _ptr(its)))
        post = {"mean": mean[:, :B], "cov": cov[:, :B]}
        return (post, its[:B].copy()) if return_iters else post

    def logit_objective(self, t, K, idx, Y, N=None, sigma=1e-3, approach="posterior", prior=None, tol=1e-5, max_iter=100,
                        return_iters=False):
        """The value train_lae_logit_gp_cpp's COBYLA minimises at t (src/train.cpp:14-34), on the resident pair with
        C = HK(idx, idx) + sigma I: approach "marginal" (-amll) or "posterior" (plus the prior, ``prior = (p, q, tau)``,
        None for PostOFData's defaults).  N None: one trial per row.  m <= K runs the dense loop of
        ``marginal_log_likelihood_logit_la``, m > K a K x K low-rank loop (include/flgp_hip.h).  sigma's default is the R
        logit wrappers'.  Returns the value, or ``(value, iters)`` with ``return_iters``."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        m = idx.size
        Y = np.ascontiguousarray(np.asarray(Y, dtype=np.float64).reshape(-1))
        if Y.size != m:
            raise ValueError("Y must have one entry per row of idx")
        N = None if N is None else np.ascontiguousarray(np.broadcast_to(np.asarray(N, dtype=np.float64), (m,)))
        pr = None if prior is None else np.ascontiguousarray(np.asarray(prior, dtype=np.float64).reshape(-1))
        if pr is not None and pr.size != 3:
            raise ValueError("prior must hold (p, q, tau)")
        value = ctypes.c_double(); it = ctypes.c_int()
        check(_lib.lib().flgp_eigenpair_logit_objective(self._h, int(K), _ptr(idx), m, _ptr(Y), _ptr(N), float(sigma),
                                                        _b(approach), _ptr(pr), float(t), float(tol), int(max_iter),
                                                        ctypes.byref(value), ctypes.byref(it)))
        return (value.value, it.value) if return_iters else value.value

    def logit_objective_batch(self, ts, K, idx, Y, col=None, N=None, sigma=1e-3, approach="posterior", prior=None, tol=1e-5,
                              max_iter=100, max_parallel=0, return_iters=False):
        """``logit_objective`` for B problems in one call (flgp_eigenpair_logit_objective_batch, include/flgp_hip.h):
        problem b is column ``col[b]`` of ``Y`` (m, or m x ncol; ``col`` None needs ncol == B and means 0 .. B-1) at
        ``ts[b]``; everything else is shared.  Each value (and iteration count) is, bit for bit, ``logit_objective`` on
        that column at that t, whatever else shares the call.  For m > K the B low-rank Newton loops advance in the same
        launches, ``max_parallel`` problems per chunk (0: as many as fit the device memory); for m <= K it is the number
        of host workers the dense loops are dealt to.  A bad ``col[b]`` or ``ts[b]`` is refused here, before the
        library is called, with the library's own text.  Returns the B values, or ``(values, iters)``."""
        who = "logit_objective_batch"
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        m = idx.size
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim > 2 or (Y.ndim == 2 and Y.shape[0] != m) or (Y.ndim < 2 and Y.size != m):
            raise ValueError("Y must have one row per entry of idx")
        Y = np.asfortranarray(Y.reshape(m, -1))
        ncol = Y.shape[1]
        ts = np.ascontiguousarray(np.asarray(ts, dtype=np.float64).reshape(-1))
        B = ts.size
        if col is None and ncol != B:
            raise FlgpError(-1, f"{who}: col may be NULL only if ncol == B (ncol={ncol}, B={B})")
        cols = None if col is None else np.ascontiguousarray(np.asarray(col, dtype=np.int32).reshape(-1))
        if cols is not None and cols.size != B:
            raise ValueError("col must have one entry per value of t")
        for b in range(B):
            c = b if cols is None else int(cols[b])
            head = "problem %d (t=%g): %s: " % (b, ts[b], who)
            if not 0 <= c < ncol:
                raise FlgpError(-1, head + "col=%d is outside [0, ncol=%d)" % (c, ncol))
            if not np.isfinite(ts[b]):
                raise FlgpError(-1, head + "t must be finite")
            if approach == "posterior" and not ts[b] > 0.0:
                raise FlgpError(-1, head + 't must be positive under "posterior"')
        N = None if N is None else np.ascontiguousarray(np.broadcast_to(np.asarray(N, dtype=np.float64), (m,)))
        pr = None if prior is None else np.ascontiguousarray(np.asarray(prior, dtype=np.float64).reshape(-1))
        if pr is not None and pr.size != 3:
            raise ValueError("prior must hold (p, q, tau)")
        values = np.zeros(max(B, 1)); its = np.zeros(max(B, 1), dtype=np.int32)
        check(_lib.lib().flgp_eigenpair_logit_objective_batch(self._h, int(K), _ptr(idx), m, _ptr(Y), ncol, _ptr(N), _ptr(cols),
                                                              _ptr(ts), B, float(sigma), _b(approach), _ptr(pr), float(tol),
                                                              int(max_iter), int(max_parallel), _ptr(values), _ptr(its)))
        values = values[:B].copy(); its = its[:B].copy()
        return (values, its) if return_iters else values

    def logit_objective_multiclass(self, ts, K, idx, labels, sigma=1e-3, approach="posterior", prior=None, tol=1e-5,
                                   max_iter=100, max_parallel=0, return_iters=False):
        """One step of train_logit_mult_gp_cpp's J one-vs-rest searches (src/MultiClassification.cpp:29-53) in one call:
        ``labels`` holds integers 0 .. J-1 (max + 1 == J, as the multiclass posterior asks), class j's response is the
        indicator column ``labels == j`` of ``multi_train_split`` with one trial per row.  ``ts``: J values (class j at
        ``ts[j]``) or a J x T array (a T-point profile per class, B = J T problems).  Returns an array of ``ts``'s shape
        whose entries are ``logit_objective`` on the class's column, bit for bit; with ``return_iters`` also the
        iteration counts in that shape."""
        lab = np.asarray(labels, dtype=np.float64).reshape(-1)
        if lab.size == 0 or not np.isfinite(lab).all() or (lab != np.floor(lab)).any() or (lab < 0).any():
            raise ValueError("labels must be class labels 0 .. J-1")
        aug_y = multi_train_split(lab)
        J = aug_y.shape[1]
        ts = np.asarray(ts, dtype=np.float64)
        if ts.ndim not in (1, 2) or ts.shape[0] != J:
            raise ValueError(f"need one t (or one row of t) per class: {J} classes, ts of shape {ts.shape}")
        T = 1 if ts.ndim == 1 else ts.shape[1]
        col = np.repeat(np.arange(J, dtype=np.int32), T)             # problem j T + k: class j at ts[j, k]
        values, its = self.logit_objective_batch(ts.reshape(-1), K, idx, aug_y, col=col, sigma=sigma, approach=approach,
                                                 prior=prior, tol=tol, max_iter=max_iter, max_parallel=max_parallel,
                                                 return_iters=True)
        values = values.reshape(ts.shape); its = its.reshape(ts.shape)
        return (values, its) if return_iters else values

    def regression_objective(self, x, K, idx, Y, sigma=1e-5, noise="same", approach="posterior", prior=None, grad=True):
        """The objective train_regression_gp_cpp minimises (src/train.cpp:333-555) and its gradient, on the resident pair:
        ``x = (t, noise)`` for noise = "same", ``(t, noise_1, ..., noise_m)`` for "different"; approach "marginal" (the
        negative marginal log likelihood) or "posterior" (plus the prior, ``prior = (p, q, tau, alpha, beta)``, None for
        PostOFDataReg's defaults).  sigma's default is the R wrappers' (R/Fit.R:56).  Returns ``(value, grad)``, or the
        value alone when ``grad=False``; the gradient is clipped as the reference clips it."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        m = idx.size
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim > 2 or (Y.ndim == 2 and Y.shape[0] != m) or (Y.ndim < 2 and Y.size != m):
            raise ValueError("Y must have one row per entry of idx")
        Y = np.asfortranarray(Y.reshape(m, -1))
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))
        pr = None if prior is None else np.ascontiguousarray(np.asarray(prior, dtype=np.float64).reshape(-1))
        if pr is not None and pr.size != 5:
            raise ValueError("prior must hold (p, q, tau, alpha, beta)")
        value = ctypes.c_double()
        g = np.zeros(x.size) if grad else None
        check(_lib.lib().flgp_eigenpair_regression_objective(self._h, int(K), _ptr(idx), m, _ptr(Y), Y.shape[1], float(sigma),
                                                             _b(noise), _b(approach), _ptr(pr), _ptr(x), x.size,
                                                             ctypes.byref(value), _ptr(g)))
        return (value.value, g) if grad else value.value

    def regression_objective_batch(self, xs, K, idx, Y, sigma=1e-5, noise="same", approach="posterior", prior=None,
                                   grad=True, max_parallel=0, return_status=False):
        """``regression_objective`` on this pair at the rows ``xs`` (A x nx) in one call: a multi-start or a line search.
        A :class:`RegressionObjectiveBatch` that lists this pair once per row, evaluated once and freed.  Returns what its
        call returns: ``(values, grads)``, each bit for bit the single call's."""
        xs = np.asarray(xs, dtype=np.float64)
        xs = xs.reshape(1, -1) if xs.ndim == 1 else xs
        ctx = RegressionObjectiveBatch([self] * xs.shape[0], K, idx, Y, sigma=sigma, noise=noise, approach=approach,
                                       prior=prior, max_parallel=max_parallel)
        try:
            return ctx(xs, grad=grad, return_status=return_status)
        finally:
            ctx.free()

    def test_pgbinary(self, idx0, idx1, K, t, Y, sigma, sigma_nv, N_sample=100, output_pi=False, seed=None,
                      return_state=False):
        """test_pgbinary_cpp (src/Predict.cpp:11-26) on the resident pair with C = HK(idx0, idx0) + sigma I: the Gibbs
        sweeps and the collapsed prediction of the rows idx1 run on the device.  ``sigma_nv`` is what the new rows'
        covariance adds where a row of idx1 is one of idx0: sigma for the binary drivers (C = [Cvv; Cnv],
        src/Fit.cpp:574-576), 0 for the one-vs-rest route.  Returns {"Y_pred"} (+ "pi_pred" with ``output_pi``, + the
        chain's final "omega" and "f" with ``return_state``)."""
        idx0 = np.ascontiguousarray(idx0, dtype=np.int32); idx1 = np.ascontiguousarray(idx1, dtype=np.int32)
        Y = np.ascontiguousarray(np.asarray(Y, dtype=np.float64).reshape(-1))
        if Y.size != idx0.size:
            raise ValueError("Y must have one entry per row of idx0")
        pi = np.zeros(idx1.size); y = np.zeros(idx1.size)
        om = np.zeros(idx0.size) if return_state else None
        f = np.zeros(idx0.size) if return_state else None
        check(_lib.lib().flgp_eigenpair_pg_predict(self._h, int(K), float(t), float(sigma), float(sigma_nv), _ptr(idx0), idx0.size,
                                                   _ptr(Y), _ptr(idx1), idx1.size, int(N_sample), _seed(seed), _ptr(pi), _ptr(y),
                                                   _ptr(om), _ptr(f)))
        out = {"Y_pred": y}
        if output_pi:
            out["pi_pred"] = pi
        if return_state:
            out["omega"] = om; out["f"] = f
        return out

    def predict_logit_mult_gp_cpp(self, idx0, idx1, K, ts, Y, sigma, N_sample=100, seed=None, output_probs=False):
        """predict_logit_mult_gp_cpp (src/MultiClassification.cpp:57-88) on the resident pair: one Polya-Gamma chain per
        class of ``multi_train_split(Y)``, class j at ``ts[j]`` with seed + j and sigma on Cvv only, then the first arg-max
        of the class probabilities.  Returns y_pred (m_new), or (y_pred, probs m_new x J) with ``output_probs``."""
        idx0 = np.ascontiguousarray(idx0, dtype=np.int32); idx1 = np.ascontiguousarray(idx1, dtype=np.int32)
        Y = np.ascontiguousarray(np.asarray(Y, dtype=np.float64).reshape(-1))
        if Y.size != idx0.size:
            raise ValueError("Y must have one entry per row of idx0")
        ts = np.ascontiguousarray(np.asarray(ts, dtype=np.float64).reshape(-1))
        J = ts.size
        probs = np.zeros((idx1.size, J), order="F"); labels = np.zeros(idx1.size)
        check(_lib.lib().flgp_eigenpair_pg_predict_multiclass(self._h, int(K), _ptr(ts), J, float(sigma), _ptr(idx0), idx0.size,
                                                              _ptr(Y), _ptr(idx1), idx1.size, int(N_sample), _seed(seed),
                                                              _ptr(probs), _ptr(labels)))
        return (labels, probs) if output_probs else labels

    def test_pgbinary_batch(self, idx0, idx1, K, ts, Y, sigma, sigma_nv, col=None, seeds=None, seed=None, N_sample=100,
                            max_parallel=0, output_pi=False, return_state=False, return_argmax=False):
        """``test_pgbinary`` for B chains in one call: chain b is column ``col[b]`` of ``Y`` (m x ncol;
        ``col=None`` needs one column per chain) at ``ts[b]`` with ``seeds[b]`` (default ``seed + b``).  For m > K the
        chains of a chunk of ``max_parallel`` (<= 0: all) share every launch of the sweep; for m <= K they are dealt to
        ``max_parallel`` workers (<= 0: min(B, 4)).  Returns the keys of ``test_pgbinary`` with a trailing chain axis
        ("Y_pred", "pi_pred": m_new x B; "omega", "f": m x B), each column ``test_pgbinary``'s bit for bit, plus "argmax"
        (m_new: the first chain with the largest pi) with ``return_argmax``."""
        who = "eigenpair_pg_predict_batch"
        idx0 = np.ascontiguousarray(idx0, dtype=np.int32); idx1 = np.ascontiguousarray(idx1, dtype=np.int32)
        m, mnew = idx0.size, idx1.size
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim > 2 or (Y.ndim == 2 and Y.shape[0] != m) or (Y.ndim < 2 and Y.size != m):
            raise ValueError("Y must have one row per entry of idx0")
        Y = np.asfortranarray(Y.reshape(m, -1))
        ncol = Y.shape[1]
        ts = np.ascontiguousarray(np.asarray(ts, dtype=np.float64).reshape(-1))
        B = ts.size
        if col is None and ncol != B:
            raise FlgpError(-1, f"{who}: col may be NULL only if ncol == B (ncol={ncol}, B={B})")
        cols = None if col is None else np.ascontiguousarray(np.asarray(col, dtype=np.int32).reshape(-1))
        if cols is not None and cols.size != B:
            raise ValueError("col must have one entry per value of t")
        if seeds is None:
            s0 = _seed(seed)
            seeds = [(s0 + b) & 0xFFFFFFFFFFFFFFFF for b in range(B)]
        seeds = np.ascontiguousarray(np.asarray([int(s) & 0xFFFFFFFFFFFFFFFF for s in np.asarray(seeds, dtype=object).reshape(-1)],
                                                dtype=np.uint64))
        if seeds.size != B:
            raise ValueError("seeds must have one entry per value of t")
        for b in range(B):
            c = b if cols is None else int(cols[b])
            head = "chain %d (t=%g, seed=%d): %s: " % (b, ts[b], int(seeds[b]), who)
            if not 0 <= c < ncol:
                raise FlgpError(-1, head + "col=%d is outside [0, ncol=%d)" % (c, ncol))
            if not np.isfinite(ts[b]):
                raise FlgpError(-1, head + "t must be finite")
        nB = max(B, 1)
        pi = np.zeros((mnew, nB), order="F"); y = np.zeros((mnew, nB), order="F")
        om = np.zeros((m, nB), order="F") if return_state else None
        f = np.zeros((m, nB), order="F") if return_state else None
        am = np.zeros(mnew) if return_argmax else None
        check(_lib.lib().flgp_eigenpair_pg_predict_batch(self._h, int(K), _ptr(idx0), m, _ptr(Y), ncol, _ptr(cols), _ptr(ts),
                                                         _ptr(seeds), B, float(sigma), float(sigma_nv), _ptr(idx1), mnew,
                                                         int(N_sample), int(max_parallel), _ptr(pi), _ptr(y), _ptr(am), _ptr(om),
                                                         _ptr(f)))
        out = {"Y_pred": y}
        if output_pi:
            out["pi_pred"] = pi
        if return_state:
            out["omega"] = om; out["f"] = f
        if return_argmax:
            out["argmax"] = am
        return out

    def predict_logit_mult_gp_batch(self, idx0, idx1, K, ts, Y, sigma, N_sample=100, seed=None, output_probs=False,
                                    max_parallel=0):
        """``predict_logit_mult_gp_cpp`` with the J = ``len(ts)`` one-vs-rest chains in one batched call: ``Y`` holds class
        labels 0 .. J-1 (a class without a member is allowed), chain j is the indicator column ``Y == j`` at ``ts[j]`` with
        seed + j and sigma on Cvv only.  Labels and probs equal ``predict_logit_mult_gp_cpp``'s bit for bit."""
        idx0 = np.ascontiguousarray(idx0, dtype=np.int32)
        lab = np.ascontiguousarray(np.asarray(Y, dtype=np.float64).reshape(-1))
        if lab.size != idx0.size:
            raise ValueError("Y must have one entry per row of idx0")
        ts = np.ascontiguousarray(np.asarray(ts, dtype=np.float64).reshape(-1))
        J = ts.size
        for a in range(lab.size):
            if not (0.0 <= lab[a] < J and lab[a] == np.floor(lab[a])):
                raise FlgpError(-1, "eigenpair_pg_predict_batch: Y[%d]=%g is not a class label in 0 .. %d" % (a, lab[a], J - 1))
        aug = (lab[:, None] == np.arange(J)[None, :]).astype(np.float64)
        out = self.test_pgbinary_batch(idx0, idx1, K, ts, aug, sigma, 0.0, seed=_seed(seed), N_sample=N_sample,
                                       max_parallel=max_parallel, output_pi=True, return_argmax=True)
        return (out["argmax"], out["pi_pred"]) if output_probs else out["argmax"]

    def to_host(self):
        values = np.zeros(self.K); vectors = np.zeros((self.n, self.K), order="F")
        check(_lib.lib().flgp_eigenpair_to_host(self._h, _ptr(values), _ptr(vectors)))
        return EigenPair(values, vectors)

    def free(self):
        if self._h is not None:
            _lib.lib().flgp_eigenpair_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def heat_kernel_spectrum_resident(X, X_new, s, r, K=-1, models=None, nstart=1, epsilon=0.1, U=None):
    """``heat_kernel_spectrum_cpp`` whose EigenPair is not copied back (see :class:`ResidentEigenPair`)."""
    models = dict(_DEFAULT_MODELS_CPP, **(models or {}))
    X = _f64(X, "X"); X_new = _f64(X_new, "X_new")
    X_all = np.asfortranarray(np.vstack([X, X_new]))
    n, d = X_all.shape
    U = _anchors(X_all, s, models, U, nstart)
    h = ctypes.c_void_p()
    check(_lib.lib().flgp_heat_kernel_spectrum_resident(_ptr(X_all), n, d, _ptr(U), s, U.shape[1], int(r), int(K),
                                                        _b(models["kernel"]), _b(models["gl"]), int(bool(models["root"])),
                                                        float(epsilon), ctypes.byref(h)))
    return ResidentEigenPair(h)


class RegressionObjectiveBatch:
    """The regression training objective for B (pair, x) problems in one call (flgp_regression_batch_*, include/flgp_hip.h;
    DESIGN 8 f-18): a context made once per bandwidth grid and called once per optimiser step.  Problem b is
    ``pairs[b]`` (a :class:`ResidentEigenPair`; a pair may be listed several times) on the shared rows ``idx``, responses
    ``Y``, ``sigma``, ``noise``, ``approach`` and ``prior``.  The pairs must outlive the context (it keeps them alive).

    ``ctx(X, prob=None, grad=True, return_status=False)``: row a of ``X`` (A x nx) is the x of problem ``prob[a]``
    (``prob`` None: problems 0 .. B-1, A == B; any order and repeats otherwise).  Returns ``(values, grads)`` of shapes
    (A,) and (A, nx), or the values alone with ``grad=False``; each entry is ``regression_objective`` on that pair at that
    x, bit for bit, whatever shares the call.  With ``return_status`` a third array holds 0 or -5 per position, a failed
    position's numbers are NaN and nothing is raised; without it the lowest failing position raises.  What the library
    would refuse about ``X`` and ``prob`` is refused here, before it is called, with its texts."""

    _WHO = "regression_objective_batch"

    def __init__(self, pairs, K, idx, Y, sigma=1e-5, noise="same", approach="posterior", prior=None, max_parallel=0):
        self._h = None
        self._pairs = list(pairs)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        m = idx.size
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim > 2 or (Y.ndim == 2 and Y.shape[0] != m) or (Y.ndim < 2 and Y.size != m):
            raise ValueError("Y must have one row per entry of idx")
        Y = np.asfortranarray(Y.reshape(m, -1))
        pr = None if prior is None else np.ascontiguousarray(np.asarray(prior, dtype=np.float64).reshape(-1))
        if pr is not None and pr.size != 5:
            raise ValueError("prior must hold (p, q, tau, alpha, beta)")
        B = len(self._pairs)
        eps = (ctypes.c_void_p * max(B, 1))(*[p._h for p in self._pairs])
        h = ctypes.c_void_p()
        check(_lib.lib().flgp_regression_batch_create(eps, B, int(K), _ptr(idx), m, _ptr(Y), Y.shape[1], float(sigma),
                                                      _b(noise), _b(approach), _ptr(pr), int(max_parallel), ctypes.byref(h)))
        self._h = h
        self._set(B, int(K), m, Y.shape[1], float(sigma), str(noise), str(approach))
        c = ctypes.c_int()
        check(_lib.lib().flgp_regression_batch_dims(self._h, None, None, None, None, None, ctypes.byref(c)))
        self.chunk = c.value

    def _set(self, B, K, m, q, sigma, noise, approach):
        self.B, self.K, self.m, self.q, self.sigma, self.noise, self.approach = B, K, m, q, sigma, noise, approach
        self.nx = m + 1 if noise == "different" else 2

    def _checked(self, X, prob):
        """X as (A, nx) C-contiguous and prob as int32 (or None), refused as the library refuses them"""
        who = self._WHO
        X = np.asarray(X, dtype=np.float64)
        X = X.reshape(1, -1) if X.ndim == 1 else X
        if X.ndim != 2 or X.shape[1] != self.nx:
            raise FlgpError(-1, '%s: noise "%s" takes %d parameters, not %d' % (who, self.noise, self.nx,
                                                                                   X.shape[-1] if X.ndim else 0))
        X = np.ascontiguousarray(X)
        A = X.shape[0]
        if A < 1:
            raise FlgpError(-1, "%s: A=%d problems" % (who, A))
        if prob is None:
            if A != self.B:
                raise FlgpError(-1, "%s: prob may be NULL only if A == B (A=%d, B=%d)" % (who, A, self.B))
        else:
            prob = np.ascontiguousarray(np.asarray(prob, dtype=np.int32).reshape(-1))
            if prob.size != A:
                raise ValueError("prob must have one entry per row of X")
        # one vectorised pass; only a call that will be refused walks the positions for the first offender, in the library's order
        ok = np.isfinite(X).all() and (X[:, 1:] + self.sigma > 0.0).all()
        ok = ok and (self.approach != "posterior" or (X[:, 0] > 0.0).all())
        ok = ok and (prob is None or ((prob >= 0) & (prob < self.B)).all())
        if ok:
            return X, prob
        for a in range(A):
            head = "position %d: %s: " % (a, who)
            if prob is not None and not 0 <= int(prob[a]) < self.B:
                raise FlgpError(-1, head + "prob=%d is outside [0, B=%d)" % (int(prob[a]), self.B))
            if not np.isfinite(X[a]).all():
                raise FlgpError(-1, head + "x must be finite")
            low = np.flatnonzero(~(X[a, 1:] + self.sigma > 0.0))
            if low.size:
                raise FlgpError(-1, head + "x[%d] + sigma must be positive" % (1 + int(low[0])))
            if self.approach == "posterior" and not X[a, 0] > 0.0:
                raise FlgpError(-1, head + 't = x[0] must be positive under "posterior"')
        return X, prob

    def __call__(self, X, prob=None, grad=True, return_status=False):
        X, prob = self._checked(X, prob)
        A = X.shape[0]
        values = np.zeros(A)
        grads = np.zeros((A, self.nx)) if grad else None
        status = np.zeros(A, dtype=np.int32) if return_status else None
        check(_lib.lib().flgp_regression_batch_eval(self._h, _ptr(prob), A, _ptr(X), self.nx, _ptr(values), _ptr(grads), self.nx,
                                                    _ptr(status)))
        out = (values, grads) if grad else (values,)
        if return_status:
            out = out + (status,)
        return out if len(out) > 1 else out[0]

    def free(self):
        if self._h is not None:
            _lib.lib().flgp_regression_batch_free(self._h)
            self._h = None
        self._pairs = []

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class LogitObjectiveBatch:
    """The logit training objective for B (pair, labels, t) problems per evaluation (flgp_logit_batch_*,
    include/flgp_hip.h): a context made once per bandwidth grid and called once per step of the t-searches.
    Problem b is ``pairs[b]`` (a :class:`ResidentEigenPair`; a pair may be listed several times) with column ``col[b]`` of
    ``Y`` (m, or m x ncol; ``col`` None needs ncol == B and means 0 .. B-1); the rows ``idx``, ``N``, ``sigma``,
    ``approach``, ``prior``, ``tol`` and ``max_iter`` are shared.  The pairs must outlive the context (it keeps them alive).

    ``ctx(ts, prob=None, return_iters=False, return_status=False)``: ``ts[a]`` is the t of problem ``prob[a]`` (``prob``
    None: problems 0 .. B-1, A == B; any order and repeats otherwise).  Returns the A values, each ``logit_objective`` on
    that pair and column at that t, bit for bit, whatever shares the call and whatever was evaluated before; with
    ``return_iters`` also the iteration counts.  With ``return_status`` a last array holds 0 or -5 per position, a failed
    position's value is NaN and nothing is raised; without it the lowest failing position raises.  What the library would
    refuse about ``ts`` and ``prob`` is refused here, before it is called, with its texts."""

    _WHO = "logit_objective_context"

    def __init__(self, pairs, K, idx, Y, col=None, N=None, sigma=1e-3, approach="posterior", prior=None, tol=1e-5,
                 max_iter=100, max_parallel=0):
        self._h = None
        self._pairs = list(pairs)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        m = idx.size
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim > 2 or (Y.ndim == 2 and Y.shape[0] != m) or (Y.ndim < 2 and Y.size != m):
            raise ValueError("Y must have one row per entry of idx")
        Y = np.asfortranarray(Y.reshape(m, -1))
        B = len(self._pairs)
        cols = None if col is None else np.ascontiguousarray(np.asarray(col, dtype=np.int32).reshape(-1))
        if cols is not None and cols.size != B:
            raise ValueError("col must have one entry per pair")
        N = None if N is None else np.ascontiguousarray(np.broadcast_to(np.asarray(N, dtype=np.float64), (m,)))
        pr = None if prior is None else np.ascontiguousarray(np.asarray(prior, dtype=np.float64).reshape(-1))
        if pr is not None and pr.size != 3:
            raise ValueError("prior must hold (p, q, tau)")
        eps = (ctypes.c_void_p * max(B, 1))(*[p._h for p in self._pairs])
        h = ctypes.c_void_p()
        check(_lib.lib().flgp_logit_batch_create(eps, _ptr(cols), B, int(K), _ptr(idx), m, _ptr(Y), Y.shape[1], _ptr(N),
                                                 float(sigma), _b(approach), _ptr(pr), float(tol), int(max_iter),
                                                 int(max_parallel), ctypes.byref(h)))
        self._h = h
        self._set(B, int(K), m, Y.shape[1], str(approach))
        P, c = ctypes.c_int(), ctypes.c_int()
        check(_lib.lib().flgp_logit_batch_dims(self._h, None, ctypes.byref(P), None, None, None, ctypes.byref(c)))
        self.P, self.chunk = P.value, c.value

    @classmethod
    def for_classes(cls, pairs, K, idx, labels, **kw):
        """The one-vs-rest grid: ``labels`` holds integers 0 .. J-1 (max + 1 == J), the columns are
        ``multi_train_split(labels)`` with one trial per row, B = P J and problem p J + j is class j on ``pairs[p]``.
        ``kw``: sigma, approach, prior, tol, max_iter, max_parallel."""
        lab = np.asarray(labels, dtype=np.float64).reshape(-1)
        if lab.size == 0 or not np.isfinite(lab).all() or (lab != np.floor(lab)).any() or (lab < 0).any():
            raise ValueError("labels must be class labels 0 .. J-1")
        aug_y = multi_train_split(lab)
        J = aug_y.shape[1]
        pairs = list(pairs)
        ctx = cls([p for p in pairs for _ in range(J)], K, idx, aug_y, col=np.tile(np.arange(J, dtype=np.int32), len(pairs)),
                  **kw)
        ctx.J = J
        return ctx

    def _set(self, B, K, m, ncol, approach):
        self.B, self.K, self.m, self.ncol, self.approach = B, K, m, ncol, approach

    def _checked(self, ts, prob):
        """ts as float64 (A,) and prob as int32 (or None), refused as the library refuses them"""
        who = self._WHO
        ts = np.ascontiguousarray(np.asarray(ts, dtype=np.float64).reshape(-1))
        A = ts.size
        if A < 1:
            raise FlgpError(-1, "%s: A=%d problems" % (who, A))
        if prob is None:
            if A != self.B:
                raise FlgpError(-1, "%s: prob may be NULL only if A == B (A=%d, B=%d)" % (who, A, self.B))
        else:
            prob = np.ascontiguousarray(np.asarray(prob, dtype=np.int32).reshape(-1))
            if prob.size != A:
                raise ValueError("prob must have one entry per value of t")
        # one vectorised pass; only a call that will be refused walks the positions for the first offender, in the library's order
        ok = np.isfinite(ts).all() and (self.approach != "posterior" or (ts > 0.0).all())
        ok = ok and (prob is None or ((prob >= 0) & (prob < self.B)).all())
        if ok:
            return ts, prob
        for a in range(A):
            head = "position %d (t=%g): %s: " % (a, ts[a], who)
            if prob is not None and not 0 <= int(prob[a]) < self.B:
                raise FlgpError(-1, head + "prob=%d is outside [0, B=%d)" % (int(prob[a]), self.B))
            if not np.isfinite(ts[a]):
                raise FlgpError(-1, head + "t must be finite")
            if self.approach == "posterior" and not ts[a] > 0.0:
                raise FlgpError(-1, head + 't must be positive under "posterior"')
        return ts, prob

    def __call__(self, ts, prob=None, return_iters=False, return_status=False):
        ts, prob = self._checked(ts, prob)
        A = ts.size
        values = np.zeros(A); its = np.zeros(A, dtype=np.int32)
        status = np.zeros(A, dtype=np.int32) if return_status else None
        check(_lib.lib().flgp_logit_batch_eval(self._h, _ptr(prob), A, _ptr(ts), _ptr(values), _ptr(its), _ptr(status)))
        out = (values,) + ((its,) if return_iters else ()) + ((status,) if return_status else ())
        return out if len(out) > 1 else out[0]

    def free(self):
        if self._h is not None:
            _lib.lib().flgp_logit_batch_free(self._h)
            self._h = None
        self._pairs = []

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class SpectrumModel:
    """A fitted graph-Laplacian spectrum (include/flgp_hip.h, "fitted spectrum model"): the anchors, the fit's two
    column-sum vectors, the cluster sizes, the anchor-side eigenpairs and sqrt(n_fit), kept on the device.  ``extend``
    runs the fit's row chain under them for rows that were not in the fit -- no eigensolve; for a row that was in the fit
    it returns that row of the fit's vectors bit for bit.  It is not a refit: refit when the new rows are a sizeable
    share of ``n_fit``.  Made by :func:`heat_kernel_spectrum_model`."""

    _GL = ("rw", "normalized", "cluster-normalized")

    def __init__(self, handle, dims=None):
        self._h = handle
        if dims is None:
            v = [ctypes.c_int() for _ in range(8)]
            check(_lib.lib().flgp_spectrum_model_dims(self._h, *[ctypes.byref(x) for x in v]))
            dims = [x.value for x in v]
        self.n_fit, self.d, self.s, self.r, self.K, kernel_se, gl, root = (int(x) for x in dims)
        self.kernel = "se" if kernel_se else "lae"
        self.gl = self._GL[gl]
        self.root = bool(root)

    @property
    def dims(self):
        return {"n_fit": self.n_fit, "d": self.d, "s": self.s, "r": self.r, "K": self.K, "kernel": self.kernel,
                "gl": self.gl, "root": self.root}

    def _handle(self):
        if self._h is None:
            raise ValueError("the spectrum model has been freed")
        return self._h

    def to_host(self):
        """The frozen state as a dict: ``values`` (K, as the pair's), ``eig`` (K, the solver's), ``V`` (s x K),
        ``colsum_gl`` (s; zeros for "rw"), ``colsum_spectrum`` (s), ``sizes`` (s; zeros unless cluster-normalized)."""
        h = self._handle()
        out = {"values": np.zeros(self.K), "eig": np.zeros(self.K), "V": np.zeros((self.s, self.K), order="F"),
               "colsum_gl": np.zeros(self.s), "colsum_spectrum": np.zeros(self.s), "sizes": np.zeros(self.s)}
        check(_lib.lib().flgp_spectrum_model_to_host(h, _ptr(out["values"]), _ptr(out["eig"]), _ptr(out["V"]),
                                                     _ptr(out["colsum_gl"]), _ptr(out["colsum_spectrum"]), _ptr(out["sizes"])))
        return out

    def extend(self, X, resident=False, head=None, head_rows=None):
        """The eigenvector rows of the points ``X`` (n_new x d): an :class:`EigenPair` with the fit's values, or with
        ``resident`` a :class:`ResidentEigenPair` whose first rows are the rows ``head_rows`` of the resident pair
        ``head`` (default: all of them) and whose last n_new rows are the extension -- one pair for the consumers, idx0
        the training rows and idx1 the new ones."""
        h = self._handle()
        X = _f64(X, "X")
        if X.shape[1] != self.d:
            raise ValueError(f"X has {X.shape[1]} columns but the model was fitted on {self.d}")
        n = X.shape[0]
        if n < 1:
            raise ValueError("X must have at least one row")
        if not resident:
            if head is not None or head_rows is not None:
                raise ValueError("head / head_rows need resident=True")
            values = np.zeros(self.K); vectors = np.zeros((n, self.K), order="F")
            check(_lib.lib().flgp_spectrum_model_extend(h, _ptr(X), n, _ptr(vectors)))
            check(_lib.lib().flgp_spectrum_model_to_host(h, _ptr(values), None, None, None, None, None))
            return EigenPair(values, vectors)
        hh, rows, n_head = None, None, 0
        if head is not None:
            if head._h is None:
                raise ValueError("the head pair has been freed")
            if head.K != self.K:
                raise ValueError(f"the head pair has K = {head.K}, the model K = {self.K}")
            rows = np.ascontiguousarray(np.arange(head.n) if head_rows is None else head_rows, dtype=np.int32).reshape(-1)
            if rows.size and (rows.min() < 0 or rows.max() >= head.n):
                raise IndexError(f"head_rows outside 0..{head.n - 1}")
            hh, n_head = head._h, rows.size
        elif head_rows is not None:
            raise ValueError("head_rows without head")
        out = ctypes.c_void_p()
        check(_lib.lib().flgp_spectrum_model_extend_resident(h, _ptr(X), n, hh, _ptr(rows) if n_head else None, n_head,
                                                             ctypes.byref(out)))
        return ResidentEigenPair(out)

    def free(self):
        if self._h is not None:
            _lib.lib().flgp_spectrum_model_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def heat_kernel_spectrum_model(X, X_new, s, r, K=-1, models=None, nstart=1, epsilon=0.1, U=None):
    """:func:`heat_kernel_spectrum_resident` that also keeps what an extension to unseen rows needs: returns
    ``(SpectrumModel, ResidentEigenPair)``, the pair bit for bit the resident entry's."""
    models = dict(_DEFAULT_MODELS_CPP, **(models or {}))
    X = _f64(X, "X"); X_new = _f64(X_new, "X_new")
    X_all = np.asfortranarray(np.vstack([X, X_new]))
    n, d = X_all.shape
    U = _anchors(X_all, s, models, U, nstart)
    hm = ctypes.c_void_p(); hp = ctypes.c_void_p()
    check(_lib.lib().flgp_heat_kernel_spectrum_model(_ptr(X_all), n, d, _ptr(U), s, U.shape[1], int(r), int(K),
                                                     _b(models["kernel"]), _b(models["gl"]), int(bool(models["root"])),
                                                     float(epsilon), ctypes.byref(hm), ctypes.byref(hp)))
    return SpectrumModel(hm), ResidentEigenPair(hp)


class Predictor:
    """A trained posterior folded into a fitted :class:`SpectrumModel` (include/flgp_hip.h, "fitted predictor"): fit
    once, then ``apply`` gives the posterior mean and variance of rows that arrive later from their r anchor weights and
    the s x (K + q) operand ``P`` -- no eigenvector rows are stored and nothing of the training is redone.  Made by
    :meth:`regression` or :meth:`logit` with the arguments of ``ResidentEigenPair.regression_posterior`` /
    ``logit_posterior_batch`` that define the trained state.  The model is borrowed and must outlive the predictor.
    :meth:`nystrom_regression` and :meth:`nystrom_logit` make the same handle over one bandwidth of a
    :class:`NystromGrid`: dense weights, the mean alone without the similarity ever going to memory.
    :meth:`pg` / :meth:`pg_for_classes` (and :meth:`nystrom_pg` / :meth:`nystrom_pg_for_classes`) fold the Polya-Gamma chains
    of ``ResidentEigenPair.test_pgbinary_batch`` instead ("Polya-Gamma predictor"): :meth:`predict` then gives the
    probabilities and labels of unseen rows; such a handle has no variance.
    A "regression" or "logit" handle also serves the joint posterior of the latent function ("joint posterior of served
    rows"): :meth:`features` and :meth:`covariance` give z_i and z_i . z_j, :meth:`draws` a handle of S seeded function draws
    per output whose :meth:`apply` returns the same functions on every call."""

    _KIND = ("regression", "logit", "pg", "draws")

    def __init__(self, handle, model, iters=None):
        self._h = handle
        self._model = model          # keeps the borrowed model (or Nystrom grid) alive
        self.iters = iters
        v = [ctypes.c_int() for _ in range(7)]
        ldp = ctypes.c_long()
        check(_lib.lib().flgp_predictor_dims(self._h, *[ctypes.byref(x) for x in v], ctypes.byref(ldp)))
        self.d, self.s, self.r, self.K, self.groups, self.q, kind = (int(x.value) for x in v)
        self.kind = self._KIND[kind]
        self.ldp = int(ldp.value)
        self.draw_shape = (1, self.q, 1) if self.kind == "draws" else None     # (groups, q, S) of the source: set by draws()

    @staticmethod
    def _trained(model, pair, idx0, Y):
        if not isinstance(model, SpectrumModel):
            raise TypeError("model must be a SpectrumModel")
        if pair._h is None:
            raise ValueError("the pair has been freed")
        idx0 = np.ascontiguousarray(idx0, dtype=np.int32).reshape(-1)
        m = idx0.size
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim > 2 or (Y.ndim == 2 and Y.shape[0] != m) or (Y.ndim < 2 and Y.size != m):
            raise ValueError("Y must have one row per entry of idx0")
        return model._handle(), idx0, m, np.asfortranarray(Y.reshape(m, -1))

    @classmethod
    def regression(cls, model, pair, Y, idx0, K, pars, sigma, noisepar="same"):
        """The regression posterior at ``pars = (t, noise ..)`` on the training rows ``idx0`` of ``pair`` (the fit's
        pair), as ``regression_posterior``; in weight space whatever m is."""
        hm, idx0, m, Y = cls._trained(model, pair, idx0, Y)
        if noisepar not in ("same", "different"):
            raise FlgpError(-3, 'predictor_regression: noisepar must be "same" or "different"')
        nz = np.ascontiguousarray(np.asarray(pars[1:], dtype=np.float64).reshape(-1))
        if noisepar == "different" and nz.size != m:
            raise ValueError('noisepar="different" needs one noise variance per training row: pars = (t, noise_1 .. noise_m)')
        if noisepar == "same":
            nz = nz[:1].copy()
        out = ctypes.c_void_p()
        check(_lib.lib().flgp_predictor_regression_create(hm, pair._h, int(K), _ptr(idx0), m, _ptr(Y), Y.shape[1], float(pars[0]),
                                                          _ptr(nz), nz.size, float(sigma), ctypes.byref(out)))
        return cls(out, model)

    @classmethod
    def logit(cls, model, pair, idx0, K, ts, Y, col=None, sigma11=0.0, sigma22=1e-3, tol=1e-5, max_iter=100, max_parallel=0):
        """The Laplace logit posteriors of B problems, as ``logit_posterior_batch``: group b of the predictor is column
        ``col[b]`` of ``Y`` at ``ts[b]``.  ``iters`` holds the Newton counts."""
        hm, idx0, m, Y = cls._trained(model, pair, idx0, Y)
        ts = np.ascontiguousarray(np.asarray(ts, dtype=np.float64).reshape(-1))
        B = ts.size
        cols = None if col is None else np.ascontiguousarray(np.asarray(col, dtype=np.int32).reshape(-1))
        if cols is not None and cols.size != B:
            raise ValueError("col must have one entry per value of t")
        its = np.zeros(max(B, 1), dtype=np.int32)
        out = ctypes.c_void_p()
        check(_lib.lib().flgp_predictor_logit_create(hm, pair._h, int(K), _ptr(idx0), m, _ptr(Y), Y.shape[1], _ptr(cols), _ptr(ts), B,
                                                     float(sigma11), float(sigma22), float(tol), int(max_iter), int(max_parallel),
                                                     _ptr(its), ctypes.byref(out)))
        return cls(out, model, its[:B].copy())

    @staticmethod
    def _trained_nystrom(grid, i, pair, idx0, Y):
        if not isinstance(grid, NystromGrid):
            raise TypeError("grid must be a NystromGrid")
        hg = grid._handle()
        i = int(i)
        if not 0 <= i < grid.l:
            raise IndexError(f"bandwidth index {i} outside 0..{grid.l - 1}")
        if pair._h is None:
            raise ValueError("the pair has been freed")
        idx0 = np.ascontiguousarray(idx0, dtype=np.int32).reshape(-1)
        m = idx0.size
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim > 2 or (Y.ndim == 2 and Y.shape[0] != m) or (Y.ndim < 2 and Y.size != m):
            raise ValueError("Y must have one row per entry of idx0")
        return hg, i, idx0, m, np.asfortranarray(Y.reshape(m, -1))

    @classmethod
    def nystrom_regression(cls, grid, i, pair, Y, idx0, K, pars, sigma, noisepar="same"):
        """:meth:`regression` over bandwidth ``i`` of a :class:`NystromGrid` (include/flgp_hip.h, "Nystrom predictor"):
        ``pair`` is the resident pair of the training rows, ``grid.extend(i, X_train, resident=True)``, and ``idx0`` its
        rows.  The grid is borrowed (the predictor keeps it alive); ``dims["r"]`` is 0: the weights are dense."""
        hg, i, idx0, m, Y = cls._trained_nystrom(grid, i, pair, idx0, Y)
        if noisepar not in ("same", "different"):
            raise FlgpError(-3, 'predictor_nystrom_regression: noisepar must be "same" or "different"')
        nz = np.ascontiguousarray(np.asarray(pars[1:], dtype=np.float64).reshape(-1))
        if noisepar == "different" and nz.size != m:
            raise ValueError('noisepar="different" needs one noise variance per training row: pars = (t, noise_1 .. noise_m)')
        if noisepar == "same":
            nz = nz[:1].copy()
        out = ctypes.c_void_p()
        check(_lib.lib().flgp_predictor_nystrom_regression_create(hg, i, pair._h, int(K), _ptr(idx0), m, _ptr(Y), Y.shape[1],
                                                                  float(pars[0]), _ptr(nz), nz.size, float(sigma), ctypes.byref(out)))
        return cls(out, grid)

    @classmethod
    def nystrom_logit(cls, grid, i, pair, idx0, K, ts, Y, col=None, sigma11=0.0, sigma22=1e-3, tol=1e-5, max_iter=100,
                      max_parallel=0):
        """:meth:`logit` over bandwidth ``i`` of a :class:`NystromGrid`; ``pair`` and ``idx0`` as in
        :meth:`nystrom_regression`."""
        hg, i, idx0, m, Y = cls._trained_nystrom(grid, i, pair, idx0, Y)
        ts = np.ascontiguousarray(np.asarray(ts, dtype=np.float64).reshape(-1))
        B = ts.size
        cols = None if col is None else np.ascontiguousarray(np.asarray(col, dtype=np.int32).reshape(-1))
        if cols is not None and cols.size != B:
            raise ValueError("col must have one entry per value of t")
        its = np.zeros(max(B, 1), dtype=np.int32)
        out = ctypes.c_void_p()
        check(_lib.lib().flgp_predictor_nystrom_logit_create(hg, i, pair._h, int(K), _ptr(idx0), m, _ptr(Y), Y.shape[1], _ptr(cols),
                                                             _ptr(ts), B, float(sigma11), float(sigma22), float(tol), int(max_iter),
                                                             int(max_parallel), _ptr(its), ctypes.byref(out)))
        return cls(out, grid, its[:B].copy())

    @staticmethod
    def _chains(who, Y, ts, col, seeds, seed):
        """ts, col, seeds of B chains with the conventions (and refusals) of ``test_pgbinary_batch``"""
        ncol = Y.shape[1]
        ts = np.ascontiguousarray(np.asarray(ts, dtype=np.float64).reshape(-1))
        B = ts.size
        if col is None and ncol != B:
            raise FlgpError(-1, f"{who}: col may be NULL only if ncol == B (ncol={ncol}, B={B})")
        cols = None if col is None else np.ascontiguousarray(np.asarray(col, dtype=np.int32).reshape(-1))
        if cols is not None and cols.size != B:
            raise ValueError("col must have one entry per value of t")
        if seeds is None:
            s0 = _seed(seed)
            seeds = [(s0 + b) & 0xFFFFFFFFFFFFFFFF for b in range(B)]
        seeds = np.ascontiguousarray(np.asarray([int(s) & 0xFFFFFFFFFFFFFFFF for s in np.asarray(seeds, dtype=object).reshape(-1)],
                                                dtype=np.uint64))
        if seeds.size != B:
            raise ValueError("seeds must have one entry per value of t")
        return ts, cols, seeds, B

    @classmethod
    def _pg(cls, create, who, head, owner, pair, idx0, m, Y, K, ts, sigma, col, seeds, seed, N_sample, max_parallel, return_state):
        ts, cols, seeds, B = cls._chains(who, Y, ts, col, seeds, seed)
        om = np.zeros((m, max(B, 1)), order="F") if return_state else None
        f = np.zeros((m, max(B, 1)), order="F") if return_state else None
        out = ctypes.c_void_p()
        check(create(*head, pair._h, int(K), _ptr(idx0), m, _ptr(Y), Y.shape[1], _ptr(cols), _ptr(ts), _ptr(seeds), B, float(sigma),
                     int(N_sample), int(max_parallel), _ptr(om), _ptr(f), ctypes.byref(out)))
        pred = cls(out, owner)
        return (pred, {"omega": om, "f": f}) if return_state else pred

    @classmethod
    def pg(cls, model, pair, idx0, K, ts, Y, sigma, col=None, seeds=None, seed=None, N_sample=100, max_parallel=0,
           return_state=False):
        """The Polya-Gamma chains of ``test_pgbinary_batch`` on the training rows ``idx0`` of ``pair``, folded into the model:
        chain b is column ``col[b]`` of ``Y`` at ``ts[b]`` with ``seeds[b]`` (default ``seed + b``).  With
        ``return_state`` returns ``(predictor, {"omega", "f"})``, the chains' final state (m x B), the batch entry's bits."""
        hm, idx0, m, Y = cls._trained(model, pair, idx0, Y)
        return cls._pg(_lib.lib().flgp_predictor_pg_create, "predictor_pg", (hm,), model, pair, idx0, m, Y, K, ts, sigma, col, seeds,
                       seed, N_sample, max_parallel, return_state)

    @staticmethod
    def _indicators(who, labels, m, J):
        lab = np.ascontiguousarray(np.asarray(labels, dtype=np.float64).reshape(-1))
        if lab.size != m:
            raise ValueError("labels must have one entry per row of idx0")
        for a in range(lab.size):
            if not (0.0 <= lab[a] < J and lab[a] == np.floor(lab[a])):
                raise FlgpError(-1, "%s: Y[%d]=%g is not a class label in 0 .. %d" % (who, a, lab[a], J - 1))
        return (lab[:, None] == np.arange(J)[None, :]).astype(np.float64)

    @classmethod
    def pg_for_classes(cls, model, pair, idx0, K, ts, labels, sigma, N_sample=100, seed=None):
        """The J = ``len(ts)`` one-vs-rest chains of ``predict_logit_mult_gp_batch``: chain j is the indicator ``labels == j``
        at ``ts[j]`` with seed + j; ``predict(X)["label"]`` is then the class of a row."""
        J = np.asarray(ts).size
        aug = cls._indicators("predictor_pg", labels, np.asarray(idx0).size, J)
        return cls.pg(model, pair, idx0, K, ts, aug, sigma, seed=_seed(seed), N_sample=N_sample)

    @classmethod
    def nystrom_pg(cls, grid, i, pair, idx0, K, ts, Y, sigma, col=None, seeds=None, seed=None, N_sample=100, max_parallel=0,
                   return_state=False):
        """:meth:`pg` over bandwidth ``i`` of a :class:`NystromGrid`; ``pair`` and ``idx0`` as in :meth:`nystrom_regression`."""
        hg, i, idx0, m, Y = cls._trained_nystrom(grid, i, pair, idx0, Y)
        return cls._pg(_lib.lib().flgp_predictor_nystrom_pg_create, "predictor_nystrom_pg", (hg, i), grid, pair, idx0, m, Y, K, ts,
                       sigma, col, seeds, seed, N_sample, max_parallel, return_state)

    @classmethod
    def nystrom_pg_for_classes(cls, grid, i, pair, idx0, K, ts, labels, sigma, N_sample=100, seed=None):
        """:meth:`pg_for_classes` over bandwidth ``i`` of a :class:`NystromGrid`."""
        J = np.asarray(ts).size
        aug = cls._indicators("predictor_nystrom_pg", labels, np.asarray(idx0).size, J)
        return cls.nystrom_pg(grid, i, pair, idx0, K, ts, aug, sigma, seed=_seed(seed), N_sample=N_sample)

    @property
    def dims(self):
        return {"d": self.d, "s": self.s, "r": self.r, "K": self.K, "groups": self.groups, "q": self.q, "kind": self.kind,
                "ldp": self.ldp}

    def _handle(self):
        if self._h is None:
            raise ValueError("the predictor has been freed")
        self._model._handle()
        return self._h

    def to_host(self):
        """``{"P": s x ldp (row-major; group g in columns g (K + q) .., its last q the mean's), "cg": groups}``.  A "pg"
        handle's P holds its q columns alone (column b chain b) and its cg is 0."""
        h = self._handle()
        out = {"P": np.zeros((self.s, self.ldp)), "cg": np.zeros(self.groups)}
        check(_lib.lib().flgp_predictor_to_host(h, _ptr(out["P"]), _ptr(out["cg"])))
        return out

    def apply(self, X, var=True):
        """The posterior of the rows ``X`` (n_new x d): ``{"mean": n_new x (groups q), "var": n_new x groups}``
        Fortran-ordered; ``var=False`` skips the variance ("var" is None) and leaves the mean's bits unchanged.  A "draws"
        handle (:meth:`draws`) returns its draws instead, one array ``n_new x groups x q x S``."""
        h = self._handle()
        X = _f64(X, "X")
        if X.shape[1] != self.d:
            raise ValueError(f"X has {X.shape[1]} columns but the model was fitted on {self.d}")
        n = X.shape[0]
        if n < 1:
            raise ValueError("X must have at least one row")
        if self.kind == "draws":
            f = np.zeros((n, self.q), order="F")
            check(_lib.lib().flgp_predictor_apply(h, _ptr(X), n, _ptr(f), None))
            return f.reshape((n,) + tuple(self.draw_shape))
        mean = np.zeros((n, self.groups * self.q), order="F")
        v = np.zeros((n, self.groups), order="F") if var else None
        check(_lib.lib().flgp_predictor_apply(h, _ptr(X), n, _ptr(mean), _ptr(v)))
        return {"mean": mean, "var": v}

    def _rows(self, X, name="X"):
        X = _f64(X, name)
        if X.shape[1] != self.d:
            raise ValueError(f"{name} has {X.shape[1]} columns but the model was fitted on {self.d}")
        if X.shape[0] < 1:
            raise ValueError(f"{name} must have at least one row")
        return X

    def _joint(self, who, group):
        """the handle of a kind that has a covariance operand, and the group index, checked before the library is touched"""
        h = self._handle()
        if self.kind not in ("regression", "logit"):
            raise FlgpError(-1, f"{who}: a handle of kind {self._KIND.index(self.kind)} has no covariance operand")
        group = int(group)
        if not 0 <= group < self.groups:
            raise IndexError(f"group {group} outside 0..{self.groups - 1}")
        return h, group

    def draws(self, S, seed):
        """A "draws" predictor of ``S`` posterior function draws per (group, output) of this "regression" or "logit" handle:
        its ``apply(X)`` returns ``n x groups x q x S`` values f(x_i) = mean_i + z_i . xi_t of the LATENT function (the diagonal
        term ``cg`` is independent noise and is left to the caller).  Draw t depends on (this handle, seed, group, output, t)
        alone -- not on S -- and a row gets the same values whenever and with whatever other rows it is served.  The new
        handle borrows the model or grid, not this predictor."""
        h, _ = self._joint("predictor_draws", 0)
        S = int(S)
        if S < 1:
            raise ValueError("S must be at least 1")
        if self.groups * self.q * S > 2 ** 31 - 16:
            raise ValueError("groups * q * S overflows an int")
        out = ctypes.c_void_p()
        check(_lib.lib().flgp_predictor_draws_create(h, S, int(seed) & 0xFFFFFFFFFFFFFFFF, ctypes.byref(out)))
        d = type(self)(out, self._model)
        d.draw_shape = (self.groups, self.q, S)
        return d

    def normals(self):
        """A "draws" handle's standard normals, ``K x ncol``: column ``(g q + c) S + t`` is ``synth.normal(seed, (g q + c) 2^32
        + t, K)``."""
        h = self._handle()
        if self.kind != "draws":
            raise FlgpError(-1, f"predictor_draws_normals: the handle is not a draws one (kind {self._KIND.index(self.kind)})")
        xi = np.zeros((self.K, self.q), order="F")
        check(_lib.lib().flgp_predictor_draws_normals(h, _ptr(xi)))
        return xi

    def features(self, X, group=0):
        """``Z`` (n x K, Fortran-ordered) with ``Z[i] = z_i`` of ``group``: the latent covariance of two rows is ``Z[i] . Z[j]``
        and ``apply``'s ``var[i, group] - cg[group]`` is ``|Z[i]|^2``."""
        h, group = self._joint("predictor_features", group)
        X = self._rows(X)
        Z = np.zeros((X.shape[0], self.K), order="F")
        check(_lib.lib().flgp_predictor_features(h, group, _ptr(X), X.shape[0], _ptr(Z)))
        return Z

    def covariance(self, Xa, Xb=None, group=0, diag_term=False):
        """The latent posterior covariance block of the rows ``Xa`` against ``Xb`` (``na x nb``, Fortran-ordered); ``Xb=None``
        means ``Xb = Xa`` and the block is exactly symmetric.  ``diag_term`` adds ``cg[group]`` on the diagonal (on the host),
        which makes the block the covariance of noisy observations; it needs ``Xb=None``."""
        h, group = self._joint("predictor_covariance", group)
        if diag_term and Xb is not None:
            raise ValueError("diag_term needs Xb=None: the diagonal term belongs to a row's covariance with itself")
        Xa = self._rows(Xa, "Xa")
        Xb = None if Xb is None else self._rows(Xb, "Xb")
        na, nb = Xa.shape[0], Xa.shape[0] if Xb is None else Xb.shape[0]
        C = np.zeros((na, nb), order="F")
        check(_lib.lib().flgp_predictor_covariance(h, group, _ptr(Xa), na, _ptr(Xb), nb, _ptr(C)))
        if diag_term:
            cg = np.zeros(self.groups)
            check(_lib.lib().flgp_predictor_to_host(h, None, _ptr(cg)))
            C[np.arange(na), np.arange(na)] += cg[group]
        return C

    def update(self, X, Y, noise=None):
        """A new "regression" predictor: this one conditioned on the newly labelled rows ``X`` (n_b x d) with responses ``Y``
        (n_b x q) -- exactly the posterior of the old and the new labels together, at the cost of the new rows alone.  ``noise``:
        None (the noise this handle was created with), one variance, or one per row.  This predictor is not modified, and the
        new one borrows the model, not this predictor.  Refused on a "logit", "pg" or "draws" handle, on a Nystrom handle and on a
        handle created with ``noisepar="different"``; a handle returned by ``update`` can always be updated again."""
        h = self._handle()
        X = self._rows(X)
        n = X.shape[0]
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim > 2 or (Y.ndim == 2 and Y.shape != (n, self.q)) or (Y.ndim < 2 and (self.q != 1 or Y.size != n)):
            raise ValueError(f"Y must have one row per row of X and q = {self.q} columns")
        Y = np.asfortranarray(Y.reshape(n, -1))
        nz = None
        if noise is not None:
            nz = np.ascontiguousarray(np.asarray(noise, dtype=np.float64).reshape(-1))
            if nz.size not in (1, n):
                raise FlgpError(-1, f"predictor_update: n_noise={nz.size} must be 0 with a NULL noise, 1 or n_b={n}")
        out = ctypes.c_void_p()
        check(_lib.lib().flgp_predictor_update(h, _ptr(X), n, _ptr(Y), _ptr(nz), 0 if nz is None else nz.size, ctypes.byref(out)))
        return type(self)(out, self._model)

    def design(self, X, B, noise=None):
        """Which ``B`` of the candidate rows ``X`` (n x d) to label next: greedy maximum-variance design.  Each step takes the
        untaken row of largest latent posterior variance given the picks so far (at equal variances the lowest row number)
        and conditions on it with observation variance ``noise + sigma``; ``noise``: None (the noise this handle was created
        with) or one variance.  Returns ``{"picks": int array (B), "gain": (B), "var": (n)}``: the 0-based rows, the latent
        variance of each at the moment it was taken, and the latent variance of every candidate after all B picks -- what
        ``update(X[picks], .)`` then serves as ``apply``'s variance minus ``cg``, whatever the labels are.  The loop this closes
        is design -> label -> ``update`` -> design again; this predictor is not modified.  Refused on the handles ``update``
        refuses."""
        h = self._handle()
        X = self._rows(X)
        n, B = X.shape[0], int(B)
        if not 1 <= B <= n:
            raise ValueError(f"B must be between 1 and the {n} rows of X")
        nz = None
        if noise is not None:
            nz = np.ascontiguousarray(np.asarray(noise, dtype=np.float64).reshape(-1))
            if nz.size != 1:
                raise ValueError("noise must be None or one variance")
        out = {"picks": np.zeros(B, dtype=np.int32), "gain": np.zeros(B), "var": np.zeros(n)}
        check(_lib.lib().flgp_predictor_design(h, _ptr(X), n, B, _ptr(nz), _ptr(out["picks"]), _ptr(out["gain"]), _ptr(out["var"])))
        return out

    def predict(self, X, latent=False):
        """A "pg" handle's answer for the rows ``X`` (n_new x d): ``{"pi": n_new x B, "y": n_new x B (pi > 0.5),
        "label": n_new (the first chain of maximal pi)}`` and, with ``latent``, ``"f"`` (pi = 1 / (1 + exp(-f)))."""
        h = self._handle()
        if self.kind != "pg":
            raise FlgpError(-1, f"predictor_pg_apply: the handle is not a Polya-Gamma one (kind {self._KIND.index(self.kind)})")
        X = _f64(X, "X")
        if X.shape[1] != self.d:
            raise ValueError(f"X has {X.shape[1]} columns but the model was fitted on {self.d}")
        n = X.shape[0]
        if n < 1:
            raise ValueError("X must have at least one row")
        out = {"pi": np.zeros((n, self.q), order="F"), "y": np.zeros((n, self.q), order="F"), "label": np.zeros(n)}
        if latent:
            out["f"] = np.zeros((n, self.q), order="F")
        check(_lib.lib().flgp_predictor_pg_apply(h, _ptr(X), n, _ptr(out.get("f")), _ptr(out["pi"]), _ptr(out["y"]), _ptr(out["label"])))
        return out

    def free(self):
        if self._h is not None:
            _lib.lib().flgp_predictor_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def nystrom_eigenpair_cpp(X, U, a2, K, resident=False):
    """The per-bandwidth block of the ``fit_nystrom_*`` drivers (reference src/Fit.cpp:244-289): Gaussian similarity
    of the anchors with the double normalisation, ``eigs_sym(W_UU, K)``, and the Nystrom extension to the rows of
    ``X``.  ``U`` is s x d (cluster-size column already dropped, as ``.leftCols(d)`` does at :242)."""
    X = _f64(X, "X"); U = _f64(U, "U")
    if X.shape[1] != U.shape[1]:
        raise ValueError("X and U must have the same number of columns")
    n, d = X.shape; s = U.shape[0]
    if resident:
        h = ctypes.c_void_p()
        check(_lib.lib().flgp_nystrom_eigenpair_resident(_ptr(X), n, d, _ptr(U), s, float(a2), int(K), ctypes.byref(h)))
        return ResidentEigenPair(h)
    values = np.zeros(int(K)); vectors = np.zeros((n, int(K)), order="F")
    check(_lib.lib().flgp_nystrom_eigenpair(_ptr(X), n, d, _ptr(U), s, float(a2), int(K), _ptr(values), _ptr(vectors)))
    return EigenPair(values, vectors)


_DEFAULT_A2S = np.exp(np.linspace(np.log(0.1), np.log(10.0), 10))      # R/Fit.R:187-189


class NystromGrid:
    """The anchor side of the ``fit_nystrom_*`` bandwidth loop (reference src/Fit.cpp:244-333) on the device, for l
    bandwidths: D_UU and its mean once, per bandwidth the top-K eigenpairs of W_UU.  ``extend`` / ``extend_all`` are the
    Nystrom extension of a row set -- no eigensolve; their results are bit for bit those of
    :func:`nystrom_eigenpair_cpp` at the same bandwidth.  Made by :func:`nystrom_spectrum_grid`."""

    def __init__(self, handle, a2s, s, d, K, workers=1):
        self._h = handle
        self.a2s = np.array(a2s, dtype=np.float64).reshape(-1)
        self.s, self.d, self.l, self.K, self.workers = int(s), int(d), self.a2s.size, int(K), int(workers)
        self._values = None
        self._mean = None

    def _handle(self):
        if self._h is None:
            raise ValueError("the Nystrom grid has been freed")
        return self._h

    def _fetch(self):
        if self._values is None:
            values = np.zeros((self.l, self.K)); mean = ctypes.c_double()
            check(_lib.lib().flgp_nystrom_grid_values(self._handle(), _ptr(values), ctypes.byref(mean)))
            self._values, self._mean = values, mean.value

    @property
    def values(self):
        """l x K: row i holds the K eigenvalues of bandwidth i, descending."""
        self._handle(); self._fetch()
        return self._values

    @property
    def distances_mean(self):
        """The mean squared distance between anchors (``distances_UU.mean()``, src/Fit.cpp:248)."""
        self._handle(); self._fetch()
        return self._mean

    def _rows(self, X):
        h = self._handle()
        X = _f64(X, "X")
        if X.shape[1] != self.d:
            raise ValueError(f"X has {X.shape[1]} columns but the grid's anchors have {self.d}")
        if X.shape[0] < 1:
            raise ValueError("X must have at least one row")
        return h, X

    def extend(self, i, X, resident=False):
        """EigenPair of bandwidth ``i`` on the rows of ``X`` (a :class:`ResidentEigenPair` with ``resident``)."""
        h, X = self._rows(X)
        i = int(i)
        if not 0 <= i < self.l:
            raise IndexError(f"bandwidth index {i} outside 0..{self.l - 1}")
        n = X.shape[0]
        if resident:
            out = ctypes.c_void_p()
            check(_lib.lib().flgp_nystrom_grid_extend_resident(h, i, _ptr(X), n, ctypes.byref(out)))
            return ResidentEigenPair(out)
        values = np.zeros(self.K); vectors = np.zeros((n, self.K), order="F")
        check(_lib.lib().flgp_nystrom_grid_extend(h, i, _ptr(X), n, _ptr(values), _ptr(vectors)))
        return EigenPair(values, vectors)

    def extend_all(self, X, resident=False):
        """The l EigenPairs on the rows of ``X`` (the training rows inside the grid): one distance pass for all
        bandwidths.  Returns a list, bandwidth i at position i."""
        h, X = self._rows(X)
        n = X.shape[0]
        if resident:
            out = (ctypes.c_void_p * self.l)()
            check(_lib.lib().flgp_nystrom_grid_extend_all_resident(h, _ptr(X), n, ctypes.addressof(out)))
            return [ResidentEigenPair(ctypes.c_void_p(out[i])) for i in range(self.l)]
        vectors = np.zeros((self.l, self.K, n))      # block i: n x K column-major
        check(_lib.lib().flgp_nystrom_grid_extend_all(h, _ptr(X), n, _ptr(vectors)))
        vals = self.values
        return [EigenPair(vals[i].copy(), np.asfortranarray(vectors[i].T)) for i in range(self.l)]

    def free(self):
        if self._h is not None:
            _lib.lib().flgp_nystrom_grid_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def nystrom_spectrum_grid(U, a2s=None, K=None, max_parallel=10):
    """The anchor side of the ``fit_nystrom_*`` drivers for the bandwidths ``a2s`` (default: the ten of R/Fit.R:187-189).
    ``U`` is s x d (cluster-size column already dropped).  Returns a :class:`NystromGrid`; see include/flgp_hip.h for
    how ``max_parallel`` is clipped; the default is the measured choice (ten concurrent dense solves: 1.6x at s = 5000,
    1.3x at s = 1e4 over one worker) and changes no bit of the result."""
    U = _f64(U, "U")
    a2s = np.ascontiguousarray(_DEFAULT_A2S if a2s is None else a2s, dtype=np.float64).reshape(-1)
    if a2s.size < 1:
        raise ValueError("a2s must hold at least one bandwidth")
    s, d = U.shape
    if K is None or not 1 <= int(K) <= s:
        raise ValueError(f"need 1 <= K <= s (K={K}, s={s})")
    h = ctypes.c_void_p()
    check(_lib.lib().flgp_nystrom_grid_create(_ptr(U), s, d, _ptr(a2s), a2s.size, int(K), int(max_parallel), ctypes.byref(h)))
    workers = ctypes.c_int()
    check(_lib.lib().flgp_nystrom_grid_dims(h, None, None, None, None, ctypes.byref(workers)))
    return NystromGrid(h, a2s, s, d, K, workers.value)


def kmeans_lloyd(X, s, init_rows, iter_max=100):
    """Lloyd k-means on the device (include/flgp_hip.h ``flgp_kmeans_lloyd``).  ``init_rows``: (nstart, s) or (s,) row
    indices of the starting centres.  Returns (U (s x (d+1), sizes last), rounds, tot_withinss)."""
    X = _f64(X, "X")
    rows = np.ascontiguousarray(np.atleast_2d(np.asarray(init_rows)), dtype=np.int32)
    if rows.shape[1] != int(s):
        raise ValueError("init_rows must hold s row indices per start")
    n, d = X.shape
    U = np.zeros((int(s), d + 1), order="F")
    it = ctypes.c_int(); wss = ctypes.c_double()
    check(_lib.lib().flgp_kmeans_lloyd(_ptr(X), n, d, int(s), _ptr(rows), rows.shape[0], int(iter_max), _ptr(U),
                                       ctypes.byref(it), ctypes.byref(wss)))
    return U, it.value, wss.value


def kmeans_minibatch(X, s, batch_size=-1, num_init=1, max_iters=100, init_fraction=-1.0, early_stop_iter=10, seed=0):
    """Mini-batch k-means on the device (include/flgp_hip.h ``flgp_kmeans_minibatch``).  Defaults = what the reference
    passes to ClusterR::MiniBatchKmeans (src/Utils.cpp:52-55: batch_size = 10 s, init_fraction = 20 s / n; the rest at
    ClusterR's defaults).  Returns (U (s x (d+1), sizes last), (iterations, winning start), tot_withinss)."""
    X = _f64(X, "X")
    n, d = X.shape
    U = np.zeros((int(s), d + 1), order="F")
    info = (ctypes.c_int * 2)(); wss = ctypes.c_double()
    check(_lib.lib().flgp_kmeans_minibatch(_ptr(X), n, d, int(s), int(batch_size), int(num_init), int(max_iters), float(init_fraction),
                                           int(early_stop_iter), int(seed), _ptr(U), ctypes.addressof(info), ctypes.byref(wss)))
    return U, (info[0], info[1]), wss.value


def subsample_cpp(X, s, method="kmeans", nstart=1, rng=None):
    """subsample_cpp (src/Utils.cpp:32-68).  ``"random"``: rows drawn without replacement (a numpy Generator in place
    of R's ``sample``).  ``"lloyd"``: k-means on the device from ``nstart`` random starts, iter.max = 100 -- same output
    contract as the reference's ``"kmeans"`` (centres + sizes), different algorithm (R's is Hartigan-Wong on R's
    RNG and cannot be reproduced outside R).  ``"kmeans"`` / ``"minibatchkmeans"`` themselves stay in R: compute the
    anchors there and pass them as ``U``."""
    X = _f64(X, "X")
    rng = np.random.default_rng(0) if rng is None else rng
    if method == "random":
        rows = rng.choice(X.shape[0], size=int(s), replace=False)
        return np.asfortranarray(X[rows, :])
    if method == "lloyd":
        rows = np.stack([rng.choice(X.shape[0], size=int(s), replace=False) for _ in range(max(1, int(nstart)))])
        return kmeans_lloyd(X, s, rows, iter_max=100)[0]
    if method == "minibatch":
        # the algorithm and parameters of the reference's "minibatchkmeans" branch (src/Utils.cpp:49-56), on the device and
        # on this library's RNG (ClusterR draws from R's: same distribution, other values)
        return kmeans_minibatch(X, s, num_init=max(1, int(nstart)), seed=int(rng.integers(0, 2**62)))[0]
    if method in ("kmeans", "minibatchkmeans"):
        raise NotImplementedError(
            f"subsample=\"{method}\" is R's stats::kmeans / ClusterR (outside the accelerated path): "
            "compute the anchors there and pass them as U (s x (d+1), cluster sizes last), or use subsample=\"lloyd\" / \"minibatch\"")
    raise FlgpError(-3, "The subsample method is not supported!")


def _anchors(X_all, s, models, U, nstart):
    if U is not None:
        U = _f64(U, "U")
        if U.shape[0] != s:
            raise ValueError(f"U has {U.shape[0]} rows but s = {s}")
        return U
    return subsample_cpp(X_all, s, models.get("subsample", "kmeans"), nstart)


def heat_kernel_spectrum_cpp(X, X_new, s, r, K=-1, models=None, nstart=1, epsilon=0.1, U=None):
    """heat_kernel_spectrum_cpp (src/Spectrum.cpp:48-76; defaults src/Spectrum.h:53-59)."""
    models = dict(_DEFAULT_MODELS_CPP, **(models or {}))
    X = _f64(X, "X"); X_new = _f64(X_new, "X_new")
    X_all = np.asfortranarray(np.vstack([X, X_new]))
    n, d = X_all.shape
    U = _anchors(X_all, s, models, U, nstart)
    Kk = s if K < 0 else int(K)
    values = np.zeros(Kk); vectors = np.zeros((n, Kk), order="F")
    check(_lib.lib().flgp_heat_kernel_spectrum(_ptr(X_all), n, d, _ptr(U), s, U.shape[1], int(r), int(K),
                                               _b(models["kernel"]), _b(models["gl"]), int(bool(models["root"])),
                                               float(epsilon), _ptr(values), _ptr(vectors)))
    return EigenPair(values, vectors)


def _devices_from_env():
    """FLGP_DEVICES="0,1,2,3": the GPUs the row-sharded entry point uses (the R shim reads the same variable)."""
    import os
    v = os.environ.get("FLGP_DEVICES", "").strip()
    if not v:
        return None
    try:
        devs = [int(x) for x in v.split(",")]
    except ValueError:
        raise FlgpError(-1, "FLGP_DEVICES=%r is not a comma-separated list of device numbers" % v) from None
    if any(x < 0 for x in devs):
        raise FlgpError(-1, "FLGP_DEVICES=%r holds a negative device number" % v)
    return devs


def heat_kernel_covariance_cpp(X, X_new, s, r, t, K, models, nstart, epsilon, U=None, devices=None):
    """heat_kernel_covariance_cpp (src/Spectrum.cpp:28-43): H is (m + m_new) x m.

    ``devices`` (or the environment variable FLGP_DEVICES) lists the GPUs to shard the rows over: the call then goes
    to ``flgp_heat_kernel_covariance_multi`` (one host thread per listed device, RCCL or the in-process transport;
    include/flgp_hip.h, "Row-sharded path").  Not an argument of the reference, which is single-process."""
    models = dict(_DEFAULT_MODELS_CPP, **(models or {}))
    X = _f64(X, "X"); X_new = _f64(X_new, "X_new")
    m = X.shape[0]
    X_all = np.asfortranarray(np.vstack([X, X_new]))
    n, d = X_all.shape
    U = _anchors(X_all, s, models, U, nstart)
    H = np.zeros((n, m), order="F")
    if devices is None:
        devices = _devices_from_env()
    if devices is not None and len(devices) >= 1:      # (a single id selects that GPU: the C entry switches to it and back)
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        check(_lib.lib().flgp_heat_kernel_covariance_multi(_ptr(X_all), n, m, d, _ptr(U), s, U.shape[1], int(r), float(t), int(K),
                                                           _b(models["kernel"]), _b(models["gl"]), int(bool(models["root"])),
                                                           float(epsilon), dev.size, _ptr(dev), _ptr(H)))
        return H
    check(_lib.lib().flgp_heat_kernel_covariance(_ptr(X_all), n, m, d, _ptr(U), s, U.shape[1], int(r), float(t), int(K),
                                                 _b(models["kernel"]), _b(models["gl"]), int(bool(models["root"])),
                                                 float(epsilon), _ptr(H)))
    return H


def heat_kernel_covariance_rcpp(X, X_new, s, r, t, K=-1, models=None, epsilon=0.1, nstart=1, U=None, devices=None):
    """heat_kernel_covariance_rcpp (R/Fit.R:760-770), with the R wrapper's defaults
    (gl="cluster-normalized", root=TRUE, K=-1)."""
    models = dict(_DEFAULT_MODELS_R, **(models or {}))
    return heat_kernel_covariance_cpp(X, X_new, s, r, t, K, models, nstart, epsilon, U=U, devices=devices)


def se_spectrum_grid(X, X_new, s, r, K=-1, a2s=None, models=None, nstart=1, U=None, max_parallel=10):
    """The spectrum part of fit_se_{regression,logit,logit_mult}_gp_cpp (src/Fit.cpp:127-178): one k-NN with
    distances, then one EigenPair per bandwidth a2 (Z = exp(-dist/(a2 mean(dist))), Laplacian, truncated SVD).
    Defaults: a2s = exp(seq(log(0.1), log(10), length.out = 10)) (R/Fit.R:128-130), models as R/Fit.R:121-124.
    Returns (list of EigenPair, distances_mean)."""
    models = dict(_DEFAULT_MODELS_R, **(models or {}))
    if a2s is None:
        a2s = np.exp(np.linspace(np.log(0.1), np.log(10.0), 10))
    a2s = np.ascontiguousarray(a2s, dtype=np.float64)
    X = _f64(X, "X"); X_new = _f64(X_new, "X_new")
    X_all = np.asfortranarray(np.vstack([X, X_new]))
    n, d = X_all.shape
    U = _anchors(X_all, s, models, U, nstart)
    Kk = s if K < 0 else int(K)
    values = np.zeros((a2s.size, Kk)); vectors = np.zeros((a2s.size, Kk, n))   # block i: n x K column-major
    mean = np.zeros(1)
    check(_lib.lib().flgp_se_spectrum_grid(_ptr(X_all), n, d, _ptr(U), s, U.shape[1], int(r), int(K), _ptr(a2s), a2s.size,
                                           _b(models["gl"]), int(bool(models["root"])), _ptr(values), _ptr(vectors),
                                           _ptr(mean), int(max_parallel)))
    return [EigenPair(values[i].copy(), np.asfortranarray(vectors[i].T)) for i in range(a2s.size)], float(mean[0])


def glgp_neighbours(threshold, n):
    """r of the sparse GLGP route: ``max(round(threshold * n), 3)`` (src/Fit.cpp:388)."""
    return int(_lib.lib().flgp_glgp_neighbours(float(threshold), int(n)))


def glgp_spectrum_grid(X, X_new, K, a2s=None, threshold=0.01, sparse=True, resident=False, max_parallel=4):
    """The spectrum step of fit_gl_{regression,logit,logit_mult}_gp_cpp (src/Fit.cpp:383-449) on the rows ``[X; X_new]``
    for the bandwidths ``a2s`` (default: the ten of R/Fit.R:227-240): the dense n x n Gaussian similarity, or with
    ``sparse`` (the R default) the one of every point's r = max(round(threshold n), 3) nearest rows, symmetrised; the two
    normalisations; the top-K eigenpairs.  n <= 32768.  Returns (list of EigenPair -- ResidentEigenPair with ``resident``
    --, distances_mean, r); see include/flgp_hip.h for the one departure from ``eigs_sym`` (largest algebraic values)."""
    a2s = np.ascontiguousarray(_DEFAULT_A2S if a2s is None else a2s, dtype=np.float64).reshape(-1)
    if a2s.size < 1:
        raise ValueError("a2s must hold at least one bandwidth")
    X = _f64(X, "X"); X_new = _f64(X_new, "X_new")
    if X.shape[1] != X_new.shape[1]:
        raise ValueError("X and X_new must have the same number of columns")
    X_all = np.asfortranarray(np.vstack([X, X_new]))
    n, d = X_all.shape
    if n < 3:
        raise ValueError(f"need at least 3 rows (n={n})")
    if K is None or not 1 <= int(K) <= n:
        raise ValueError(f"need 1 <= K <= n (K={K}, n={n})")
    K = int(K); l = a2s.size
    if sparse and not (np.isfinite(threshold) and threshold > 0):
        raise ValueError(f"threshold must be positive and finite (got {threshold})")
    if sparse and np.floor(float(threshold) * n + 0.5) > n:
        raise ValueError(f"threshold {threshold} asks for more than n = {n} neighbours")
    mean = ctypes.c_double(); r = ctypes.c_int()
    L = _lib.lib()
    if resident:
        out = (ctypes.c_void_p * l)()
        check(L.flgp_glgp_spectrum_grid(_ptr(X_all), n, d, K, _ptr(a2s), l, int(bool(sparse)), float(threshold), int(max_parallel),
                                        None, None, ctypes.addressof(out), ctypes.byref(mean), ctypes.byref(r)))
        pairs = [ResidentEigenPair(ctypes.c_void_p(out[i])) for i in range(l)]
    else:
        values = np.zeros((l, K)); vectors = np.zeros((l, K, n))      # block i: n x K column-major
        check(L.flgp_glgp_spectrum_grid(_ptr(X_all), n, d, K, _ptr(a2s), l, int(bool(sparse)), float(threshold), int(max_parallel),
                                        _ptr(values), _ptr(vectors), None, ctypes.byref(mean), ctypes.byref(r)))
        pairs = [EigenPair(values[i].copy(), np.asfortranarray(vectors[i].T)) for i in range(l)]
    return pairs, mean.value, r.value


def lae_eigenmap(X, s, r=3, ndim=2, subsample="kmeans", norm="cluster-normalized", nstart=1, U=None):
    """lae_eigenmap (src/Spectrum.cpp:17-25, defaults src/Spectrum.h:43-44)."""
    X = _f64(X, "X")
    n, d = X.shape
    U = _anchors(X, s, dict(subsample=subsample), U, nstart)
    ev = np.zeros(int(ndim)); vec = np.zeros((n, int(ndim)), order="F")
    check(_lib.lib().flgp_lae_eigenmap(_ptr(X), n, d, _ptr(U), s, U.shape[1], int(r), int(ndim), _b(norm), _ptr(ev), _ptr(vec)))
    return {"eigenvalues": ev, "eigenvectors": vec}
