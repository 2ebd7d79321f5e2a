"""Plain-numpy yardstick of the TV-Lp prox for general p, independent of the library (not a test module).

    P(x) = 1/2 ||x - y||^2 + lam ||Dx||_p          the primal, D the forward difference
    D(u) = u'Dy - 1/2 ||D'u||^2 , ||u||_q <= lam   the dual, q = p / (p - 1) ; x = y - D'u at the optimum

tvp_gap(x, y, lam, p) = P(x) - D(u) with u = cumsum(x - y)[:-1] scaled into the q-ball: for ANY x an upper bound on P(x) - P*, and
so, P being 1-strongly convex, ||x - x*||_2 <= sqrt(2 tvp_gap)."""
import numpy as np


def lp_norm(v, p):
    """||v||_p for 1 <= p <= inf, without overflow for large p."""
    v = np.abs(np.asarray(v, dtype=np.float64)).ravel()
    if v.size == 0:
        return 0.0
    m = float(v.max())
    if m == 0.0 or np.isinf(p):
        return m
    return m * float(np.sum((v / m) ** p)) ** (1.0 / p)


def dual_exponent(p):
    if p == 1:
        return np.inf
    if np.isinf(p):
        return 1.0
    return p / (p - 1.0)


def primal(x, y, lam, p):
    x, y = np.asarray(x, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel()
    return 0.5 * float(np.sum((x - y) ** 2)) + lam * lp_norm(np.diff(x), p)


def dual_point(x, y, lam, p):
    """u = cumsum(x - y)[:-1], scaled into the ball ||u||_q <= lam."""
    x, y = np.asarray(x, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel()
    u = np.cumsum(x - y)[:-1]
    nu = lp_norm(u, dual_exponent(p))
    if nu > lam:
        u = u * (lam / nu)
    return u


def dual(u, y):
    y = np.asarray(y, dtype=np.float64).ravel()
    dtu = np.concatenate([[0.0], u]) - np.concatenate([u, [0.0]])     # (D'u)_i = u_{i-1} - u_i
    return float(np.dot(u, np.diff(y))) - 0.5 * float(np.sum(dtu ** 2))


def tvp_gap(x, y, lam, p):
    x, y = np.asarray(x, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel()
    if x.size < 2:
        return 0.5 * float(np.sum((x - y) ** 2))
    return primal(x, y, lam, p) - dual(dual_point(x, y, lam, p), y)


def radius(x, y, lam, p):
    """sqrt(2 tvp_gap): the bound on ||x - x*||_2 (a gap that rounding left a hair below zero counts as zero)."""
    return float(np.sqrt(2.0 * max(tvp_gap(x, y, lam, p), 0.0)))


def signal(n, seed):
    """The 1-D family of the goldens: standard normal plus a step of 2 at the middle."""
    y = np.random.default_rng(seed).standard_normal(n)
    y[n // 2:] += 2.0
    return y


# the 1-D grid of tests/golden/golden_pgen.npz: (n, p, lam)
GRID = [(n, p, lam) for n in (2, 3, 17, 100, 1000) for p in (1.5, 3.0, 7.0, 20.0) for lam in (0.05, 1.0, 30.0)
        if (n, p, lam) != (1000, 1.5, 30.0)] + [(n, 1.1, lam) for n in (2, 3, 17, 100, 1000) for lam in (0.05, 1.0)]
