"""CPU: the classification entries (include/flgp_hip.h) refuse bad labels and shapes before any device
work, so these run without a GPU."""
import numpy as np
import pytest

from flgp_amd import _lib, api


def test_classification_symbols_are_bound():
    L = _lib.lib()
    for name in ("flgp_logit_la_marginal_likelihood", "flgp_eigenpair_logit_marginal_likelihood",
                 "flgp_eigenpair_posterior_classification", "flgp_dev_cholesky", "flgp_dev_chol_solve"):
        assert hasattr(L, name)


@pytest.mark.parametrize("Y,N,what", [
    ([0.0, 2.0, 1.0], [1.0, 1.0, 1.0], "outside"),       # Y > N
    ([0.0, -1.0, 1.0], [1.0, 1.0, 1.0], "outside"),      # Y < 0
    ([0.0, 1.0, 1.0], [1.0, 0.0, 1.0], "positive"),      # N = 0
    ([0.0, np.nan, 1.0], [1.0, 1.0, 1.0], "outside"),    # NaN label
])
def test_bad_labels_are_refused(Y, N, what):
    with pytest.raises(api.FlgpError) as e:
        api.marginal_log_likelihood_logit_la_cpp(np.eye(3), Y, N)
    assert e.value.code == -1 and what in e.value.message


def test_bad_shapes_are_refused():
    with pytest.raises(api.FlgpError) as e:
        api.marginal_log_likelihood_logit_la_cpp(np.eye(3), [0, 1, 0], 1, max_iter=0)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        api.marginal_log_likelihood_logit_la_cpp(np.eye(3), [0, 1], 1)


def test_multi_train_split():
    aug = api.multi_train_split(np.array([2, 0, 1, 2]))
    np.testing.assert_array_equal(aug, [[0, 0, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
