"""CPU: the algebra of the Nystrom predictor (tests/np_nystrom_predictor.py) on random operands: the folded
row z_i = f_i sum_j Z_ij P_j equals [G ; U^T] u_i on the extension's row u_i, to rounding, in float64 and np.longdouble."""
import numpy as np
import pytest

import np_nystrom_predictor as nnp


@pytest.mark.parametrize("dtype,rtol", [(np.float64, 1e-12), (np.longdouble, 1e-15)])
@pytest.mark.parametrize("n,d,s,K,q,groups", [(37, 3, 20, 5, 1, 1), (50, 9, 70, 12, 3, 2), (9, 40, 65, 64, 2, 3)])
def test_fold_then_rows_is_the_operand_on_the_extended_row(n, d, s, K, q, groups, dtype, rtol):
    rng = np.random.default_rng([n, d, s, K])
    X = rng.normal(size=(n, d)); U = rng.normal(size=(s, d))
    inv_c = 1.0 / (0.7 * 2.0 * d)
    w = rng.uniform(0.01, 0.1, s)
    Vp = rng.normal(size=(s, K))
    ops = [(rng.normal(size=(K, K)), rng.normal(size=(K, q))) for _ in range(groups)]
    cg = rng.uniform(1e-3, 1.0, groups)
    P = np.hstack([nnp.fold(Vp.astype(dtype), G.astype(dtype), Uo.astype(dtype)) for G, Uo in ops])
    assert P.shape == (s, groups * (K + q))
    mean, var = nnp.rows(X, U, inv_c, w, P, groups, K, q, cg, dtype)
    u = nnp.extend(X, U, inv_c, w, Vp, dtype)
    assert np.isfinite(u).all() and np.abs(u).max() > 0
    for g, (G, Uo) in enumerate(ops):
        want_mean = u @ Uo.astype(dtype)
        want_var = dtype(cg[g]) + ((u @ G.astype(dtype).T) ** 2).sum(1)
        scale = np.abs(u) @ np.abs(Uo)
        assert (np.abs(mean[:, g * q:(g + 1) * q] - want_mean) <= rtol * scale).all()
        assert (np.abs(var[:, g] - want_var) <= rtol * ((np.abs(u) @ np.abs(G.T)) ** 2).sum(1) + rtol * cg[g]).all()
        assert (var[:, g] >= cg[g]).all()


def test_the_row_factor_is_the_extensions():
    """f as nys_factor_kernel writes it, against W_XU = A_XU / (rowsum(A_XU) + 1e-9) with A_XU = Z / (rs_X rs_U^T) spelled out"""
    rng = np.random.default_rng(4)
    X = rng.normal(size=(30, 4)); U = rng.normal(size=(11, 4))
    Z = nnp.similarity(X, U, 0.2)
    w = 1.0 / (rng.uniform(1.0, 5.0, 11) + 1e-9)
    A = Z / (Z.sum(1) + 1e-9)[:, None] * w[None, :]
    W = A / (A.sum(1) + 1e-9)[:, None]
    np.testing.assert_allclose(nnp.row_factor(Z, w)[:, None] * Z * w[None, :], W, rtol=1e-13)
