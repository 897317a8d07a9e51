"""What tests/test_gpu_predictor_pg.py and tests/test_gpu_nystrom_predictor_pg.py assert of a prediction against the batch
entry's (the derivation: the former's docstring): tol_pi from the reference alone, and the rows on which y and label must
agree -- all of them, which is asserted on the reference."""
import numpy as np

import regression_posterior_cases as rc

U8 = 8.0 * 2.0 ** -53


def bounds(pi_ref, duplicates=()):
    """tol_pi from the batch entry's output, and the assertion that every row is on the safe side for y and label"""
    with np.errstate(divide="ignore"):
        F = np.abs(np.log(pi_ref / (1.0 - pi_ref))).max()
    assert 0.0 < F < 20.0, F
    tol = 0.25 * rc.atol_mean(np.array([F])) + U8
    assert (np.abs(pi_ref - 0.5) > tol).all()
    B = pi_ref.shape[1]
    same = {b: {b} for b in range(B)}
    for a, c in duplicates:
        same[a].add(c); same[c].add(a)
    if any(len(v) < B for v in same.values()):
        first = np.argmax(pi_ref, axis=1)
        rest = np.array(pi_ref)
        for i, b in enumerate(first):
            rest[i, sorted(same[b])] = -np.inf
        assert (pi_ref.max(axis=1) - rest.max(axis=1) > 2.0 * tol).all()
    return tol


def compare(got, ref, label, duplicates=((0, 2),)):
    """got: predict(..); ref: test_pgbinary_batch(.., output_pi, return_argmax).  Returns |d| / tol_pi"""
    tol = bounds(ref["pi_pred"], duplicates)
    d = np.abs(got["pi"] - ref["pi_pred"]).max()
    print(f"{label}: max |f_ref| {np.abs(np.log(ref['pi_pred'] / (1.0 - ref['pi_pred']))).max():.2f}; "
          f"|pi - pi_ref| {d:.3e} bound {tol:.3e} ratio {d / tol:.3e}")
    assert d <= tol
    np.testing.assert_array_equal(got["y"], ref["Y_pred"])
    np.testing.assert_array_equal(got["label"], ref["argmax"])
    np.testing.assert_array_equal(got["y"], (got["pi"] > 0.5).astype(float))
    return d / tol
