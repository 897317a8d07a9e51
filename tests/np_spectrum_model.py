"""The fitted spectrum model's extension (flgp_amd/csrc/model.hip) restated from pieces that are each
pinned already: the compiled oracle's k-NN and LAE, then the numpy restatements of tests/np_sparse_stages.py, one rounded
operation at a time, under GIVEN column sums, cluster sizes and anchor-side eigenpairs.  tests/test_spectrum_model_args.py
anchors it to the oracle's own pipeline on the CPU; tests/test_gpu_spectrum_model.py holds the device to it bit for bit."""
import math

import numpy as np

import np_sparse_stages as nps

GLS = ("rw", "normalized", "cluster-normalized")


def scale(idx, val, colsum_gl, sizes, colsum_spectrum):
    """flgp_dev_extend_scale as the fit's three passes: col_scale(mode 0) (not where colsum_gl is None: "rw"), row_normalize,
    col_scale(mode 1)."""
    if colsum_gl is not None:
        val = nps.col_scale(idx, val, colsum_gl, sizes, 0)
    val = nps.row_normalize(val)
    return nps.col_scale(idx, val, colsum_spectrum, None, 1)


def extend(X, U0, r, gl, colsum_gl, colsum_spectrum, sizes, V, eig, n_fit, root=False):
    """The rows X through the chain of a fit on n_fit rows with anchors U0 (s x d): the oracle's k-NN and LAE, the three
    scalings under the fit's sums, u = a V / sigma * sqrt(n_fit).  Returns (vectors n x K, values K)."""
    from oracle import flgp_oracle as O
    assert gl in GLS
    X = np.asfortranarray(X, dtype=np.float64); U0 = np.asfortranarray(U0, dtype=np.float64)
    idx, z = O.lae(X, U0, r, knn_idx=O.knn(X, U0, r))
    a = scale(idx, z, None if gl == "rw" else colsum_gl, sizes if gl == "cluster-normalized" else None, colsum_spectrum)
    return nps.u_recover(idx, a, V, eig, math.sqrt(float(n_fit)), root)


def oracle_fit(X, U, r, K, gl, root=False):
    """A fit from the oracle's stages alone, Gram route (the device's): what a model freezes, and the fit's vectors.
    U: s x d, or s x (d+1) with the cluster sizes last.  Returns a dict with colsum_gl (None for "rw"), colsum_spectrum,
    sizes (None unless cluster-normalized), V (s x K), eig (K), values, vectors (n x K)."""
    from oracle import flgp_oracle as O
    X = np.asfortranarray(X, dtype=np.float64)
    n, d = X.shape
    s = U.shape[0]
    U0 = np.asfortranarray(U[:, :d])
    sizes = np.ascontiguousarray(U[:, d]) if gl == "cluster-normalized" else None
    idx, z = O.lae(X, U0, r)
    colsum_gl = None if gl == "rw" else O.colsum(idx, z, s)
    zn = O.graph_laplacian(idx, z, s, gl, sizes)
    a, colsum_spectrum = O.scale_A(idx, zn, s)
    w, V = np.linalg.eigh(O.gram(idx, a, s))
    eig = w[::-1][:K].copy(); V = np.asfortranarray(V[:, ::-1][:, :K])
    sigma = np.sqrt(np.maximum(eig, 0.0))
    return {"colsum_gl": colsum_gl, "colsum_spectrum": colsum_spectrum, "sizes": sizes, "V": V, "eig": eig,
            "values": sigma if root else eig, "vectors": O.u_recover(idx, a, s, V, sigma), "U0": U0}
