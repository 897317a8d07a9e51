"""numpy restatement of the predictive negative log likelihood (flgp_amd/csrc/nll.hip; reference src/Utils.cpp:302-336)
on the random numbers the device consumes: class j draws from stream j, and row i's samples are
synth.normal(seed, j, n_samples, offset=i * n_samples), so a handful of rows of a large problem can be regenerated."""
import numpy as np

from flgp_amd import synth


def logistic(f):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-f))


def like_from_normals(mean, cov, y01, z):
    """the per-row Monte-Carlo likelihoods of nll_classification from the normals z (rows x n_samples)"""
    with np.errstate(invalid="ignore"):
        f = mean[:, None] + np.sqrt(cov)[:, None] * z
    pi = logistic(f)
    return (pi * y01[:, None] + (1.0 - pi) * (1.0 - y01[:, None])).mean(axis=1)


def like_rows(mean, cov, y01, n_samples, seed, stream, rows=None):
    """like of the rows `rows` (None: all of them) of the problem (mean, cov, y01) under (seed, stream)"""
    mean = np.asarray(mean, dtype=np.float64); cov = np.asarray(cov, dtype=np.float64); y01 = np.asarray(y01, dtype=np.float64)
    if rows is None:       # every row: one call gives the same numbers as a call per row
        z = synth.normal(seed, stream, mean.size * n_samples).reshape(mean.size, n_samples)
        return like_from_normals(mean, cov, y01, z)
    rows = np.asarray(rows)
    z = np.stack([synth.normal(seed, stream, n_samples, offset=int(i) * n_samples) for i in rows])
    return like_from_normals(mean[rows], cov[rows], y01[rows], z)


def value_from_like(like):
    return -np.mean(np.log(like + 1e-2))


def nll_classification(mean, cov, y01, n_samples, seed, stream=0):
    """(value, like) of one class"""
    like = like_rows(mean, cov, y01, n_samples, seed, stream)
    return value_from_like(like), like


def nll_multinomial(mean, cov, labels, n_samples, seed):
    """(value, like n x J): the class values added in class order from 0.0, class j on stream j"""
    labels = np.asarray(labels).reshape(-1)
    J = mean.shape[1]
    like = np.zeros(mean.shape, order="F")
    value = 0.0
    for j in range(J):
        v, like[:, j] = nll_classification(mean[:, j], cov[:, j], (labels == j).astype(np.float64), n_samples, seed, j)
        value += v
    return value, like


def nll_regression(mean, cov, y):
    """(value, per-row terms), with the reference's truncated constant"""
    terms = (y - mean) ** 2 / cov + np.log(cov + 1e-9)
    return (terms.mean() + np.log(2 * 3.1415926)) / 2, terms


def inputs(n, seed, J=None):
    """mean ~ 3 N(0, 1), sqrt(cov) ~ U(0, 4), targets drawn from logistic(mean) (J: labels by the columns' softmax)"""
    rng = np.random.default_rng(seed)
    shape = (n,) if J is None else (n, J)
    mean = np.asfortranarray(3.0 * rng.standard_normal(shape))
    cov = np.asfortranarray(rng.uniform(0.0, 4.0, shape) ** 2)
    if J is None:
        return mean, cov, (rng.uniform(size=n) < logistic(mean)).astype(np.float64)
    p = np.exp(mean - mean.max(axis=1, keepdims=True))
    c = np.cumsum(p / p.sum(axis=1, keepdims=True), axis=1)
    labels = np.minimum((rng.uniform(size=n)[:, None] > c).sum(axis=1), J - 1).astype(np.float64)
    labels[:J] = np.arange(J)        # every class present, so that max(label) + 1 == J at any n >= J
    return mean, cov, labels
