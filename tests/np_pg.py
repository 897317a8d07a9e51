"""A numpy restatement of the Polya-Gamma Gibbs sampler on the device (flgp_amd/csrc/pg.hip, include/flgp_hip.h): the same
PG(1, z) algorithm and the same random numbers (flgp_amd/synth.py, with the stream layout pg.hip documents), so that the
device's omega, f and pi can be reproduced to rounding.  Dense linear algebra throughout: it restates the law of
PGLogitModel (reference src/PGLogitModel.cpp) in Matheron's form, not the device's routes."""
import numpy as np
from scipy.special import erfc, erfcx

from flgp_amd import synth

T = 0.64


def _log_phi(x):
    if x < 0.0:
        return np.log(0.5 * erfcx(-x * np.sqrt(0.5))) - 0.5 * x * x
    return np.log(0.5 * erfc(-x * np.sqrt(0.5)))


def _a(n, x):
    k = n + 0.5
    if x <= T:
        return np.pi * k * (2.0 / (np.pi * x)) ** 1.5 * np.exp(-2.0 * k * k / x)
    return np.pi * k * np.exp(-0.5 * k * k * np.pi * np.pi * x)


class _Ctr:
    def __init__(self, seed, stream, entry):
        self.seed, self.stream, self.q0, self.q = seed, stream, entry << 32, 0

    def next(self):
        u = synth.uniform(self.seed, self.stream, 1, self.q0 + self.q)[0]
        self.q += 1
        return u


def jstar(z, r):
    t = T
    K = np.pi ** 2 / 8.0 + 0.5 * z * z
    lp = np.log(np.pi / (2.0 * K)) - K * t
    l1 = -z + _log_phi((t * z - 1.0) / np.sqrt(t))
    l2 = z + _log_phi(-(t * z + 1.0) / np.sqrt(t))
    lq = np.log(2.0) + max(l1, l2) + np.log1p(np.exp(-abs(l1 - l2)))
    with np.errstate(over="ignore"):
        p_right = 1.0 / (1.0 + np.exp(lq - lp))       # 0 once the left proposal dominates beyond double range
    mu = np.inf if z == 0 else 1.0 / z
    while True:
        if r.next() < p_right:
            X = t + (-np.log(r.next())) / K
        elif mu > t:
            while True:
                while True:
                    E1 = -np.log(r.next()); E2 = -np.log(r.next())
                    if E1 * E1 <= 2.0 * E2 / t:
                        break
                d = 1.0 + t * E1
                X = t / (d * d)
                if r.next() <= np.exp(-0.5 * z * z * X):
                    break
        else:
            while True:
                u1 = r.next(); u2 = r.next()
                nr = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
                a = mu * (nr * nr)
                X = mu / (1.0 + 0.5 * a + 0.5 * np.sqrt(a * a + 4.0 * a))
                if r.next() > mu / (mu + X):
                    X = mu * mu / X
                if X < t:
                    break
        S = _a(0, X)
        Y = r.next() * S
        n = 1
        while True:
            an = _a(n, X)
            if n & 1:
                S -= an
                if Y <= S:
                    return X
            else:
                S += an
                if Y > S:
                    break
            n += 1


def pg_draw(c, seed, stream, b=None):
    out = np.zeros(len(c))
    for i, ci in enumerate(c):
        r = _Ctr(seed, stream, i)
        nb = 1 if b is None else int(b[i])
        s = 0.0
        for _ in range(nb):
            s += 0.25 * jstar(0.5 * abs(ci), r)
        out[i] = s
    return out


def chain(Y, n_sample, seed, sigma=None, V1=None, l=None, ls=None, C=None):
    """PGLogitModel's sweeps in Matheron's form.  Eigen form: C = V1 diag(l) V1^T + sigma I with f0 = V1 (ls z1) +
    sqrt(sigma) z2; dense form (V1 None): the given C with f0 = chol(C) z2.  Returns (omega, f, kappa, C, cmul)."""
    m = Y.size
    kappa = Y - 0.5
    omega = np.ones(m)
    f = np.zeros(m)
    if V1 is not None:
        K = V1.shape[1]
        C = V1 @ (l[:, None] * V1.T) + sigma * np.eye(m)

        def cmul(x):
            return V1 @ (l * (V1.T @ x)) + sigma * x
    else:
        K = 0
        LC = np.linalg.cholesky(C)

        def cmul(x):
            return C @ x
    for s in range(n_sample):
        z2 = synth.normal(seed, 4 * s + 1, m)
        z3 = synth.normal(seed, 4 * s + 2, m)
        if V1 is not None:
            z1 = synth.normal(seed, 4 * s, K)
            f0 = V1 @ (ls * z1) + np.sqrt(sigma) * z2
        else:
            f0 = LC @ z2
        sw = np.sqrt(omega)
        r = kappa / sw - sw * f0 - z3
        B = sw[:, None] * C * sw[None, :] + np.eye(m)
        x = sw * np.linalg.solve(B, r)
        f = f0 + cmul(x)
        omega = pg_draw(f, seed, 4 * s + 3)
    return omega, f, kappa, C, cmul


def collapsed_w(omega, kappa, C):
    """w = kappa - sqrt(omega) B^-1 sqrt(omega) C kappa (src/PGLogitModel.cpp:61-73)"""
    sw = np.sqrt(omega)
    B = sw[:, None] * C * sw[None, :] + np.eye(omega.size)
    return kappa - sw * np.linalg.solve(B, sw * (C @ kappa))


def logistic(x):
    return 1.0 / (1.0 + np.exp(-x))


def weights(values, K, t):
    lam = 1.0 - values[:K]
    return np.exp(-t * lam), np.exp(-0.5 * t * lam)
