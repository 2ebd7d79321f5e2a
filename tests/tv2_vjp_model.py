"""Plain-numpy model of the derivative of the 1-D TV-L2 prox (what proxtv_tv2_fibres_vjp_dev computes), shared by
tests/test_tv2_vjp_host.py and tests/test_gpu_tv2_vjp.py.  Not a test module.

Per fibre of n samples: D the (n-1) x n difference matrix, T = D D' = tridiag(-1, 2, -1), y = prox(x) = x - D'u.  Either u = T^-1 D x
lies inside the ball ||u|| <= lambda (mu = 0, y the mean of x) or (T + mu I) u = D x with ||u|| = lambda, and then D y = mu u, so
mu = ||D y|| / lambda.  With M = T + mu I, a cotangent g and h = D g:
    active   p = M^-1 h, q = M^-1 (D y), kappa = h'q / (D y)'q, gx = g - D'(p - kappa q), glam = -mu lambda kappa
    inside   gx = mean(g), glam = 0
    n == 1 or lambda <= 0: gx = g, glam = 0
"""
import numpy as np

LENGTHS = (1, 2, 3, 7, 64, 65, 129)
LAMBDAS = (0.05, 0.8, 3.0, 40.0)
KINK_BAND = 0.05          # central differences straddle the kink when | ||T^-1 D x|| - lambda | < 0.05 lambda
# unit-normal data drawn in the order of cases().  The seed is a choice of inputs: with it ||T^-1 D x|| is at least KINK_CLEAR away from
# lambda in every case (tests/test_tv2_vjp_host.py asserts that), so none lies in the kink band, and the one case whose multiplier could
# be tiny -- n = 129 at lambda = 40, where an active fibre has mu ~ 1e-4 to 1e-3, of the size of T's smallest eigenvalue, and central
# differences with h = 1e-5 feel the kink's curvature (8e-9 .. 2e-8 on such draws) -- lies inside the ball
SEED = 30
KINK_CLEAR = 0.2


def tmat(n, mu=0.0):
    """T + mu I for a fibre of n samples, dense."""
    m = n - 1
    return (2.0 + mu) * np.eye(m) - np.eye(m, k=1) - np.eye(m, k=-1)


def solve(n, mu, rhs, banded=False):
    """(T + mu I)^-1 rhs: dense, or (long fibres) banded -- scipy's Cholesky where scipy is installed, else an LDL' sweep."""
    if not banded:
        return np.linalg.solve(tmat(n, mu), rhs)
    try:
        from scipy.linalg import solveh_banded
        ab = np.empty((2, n - 1))
        ab[0], ab[1] = -1.0, 2.0 + mu
        return solveh_banded(ab, rhs)
    except ImportError:
        m = n - 1
        d, z = np.empty(m), np.empty(m)
        d[0], z[0] = 2.0 + mu, rhs[0]
        for i in range(1, m):
            d[i] = 2.0 + mu - 1.0 / d[i - 1]
            z[i] = rhs[i] + z[i - 1] / d[i - 1]
        out = np.empty(m)
        out[-1] = z[-1] / d[-1]
        for i in range(m - 2, -1, -1):
            out[i] = (z[i] + out[i + 1]) / d[i]
        return out


def dual_norm(x, banded=False):
    """||T^-1 D x||: what the branch is decided by."""
    x = np.asarray(x, dtype=np.float64)
    return float(np.linalg.norm(solve(x.size, 0.0, np.diff(x), banded))) if x.size > 1 else 0.0


def mu_of(x, y, lam, banded=False):
    """(mu, ||T^-1 D x||) of one fibre: mu = 0 inside the ball (and for n == 1, lambda <= 0), else ||D y|| / lambda."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if x.size < 2 or not lam > 0:
        return 0.0, 0.0
    un = dual_norm(x, banded)
    return (0.0 if un <= lam else float(np.linalg.norm(np.diff(y))) / lam), un


def near_kink(unorm, lam):
    return abs(unorm - lam) < KINK_BAND * lam


def vjp_1d(y, mu, g, lam, banded=False):
    """(gx, glam) of one fibre from the prox's output y and its multiplier mu."""
    y, g = np.asarray(y, dtype=np.float64), np.asarray(g, dtype=np.float64)
    n = y.size
    if n < 2 or not lam > 0:
        return g.copy(), 0.0
    if not mu > 0:
        return np.full(n, g.mean()), 0.0
    dy, h = np.diff(y), np.diff(g)
    p, q = solve(n, mu, h, banded), solve(n, mu, dy, banded)
    kappa = float(h @ q) / float(dy @ q)
    w = p - kappa * q
    gx = g.copy()          # g - D'w: (D'w)_i = w_{i-1} - w_i
    gx[:-1] += w
    gx[1:] -= w
    return gx, -mu * lam * kappa


def vjp_nd(y, mu, g, lam, dim):
    """The same along `dim` of an N-D array; mu and the returned glam in the column-major order of the array with `dim` removed."""
    ym, gm = np.moveaxis(y, dim, -1), np.moveaxis(g, dim, -1)
    mum = np.asarray(mu, dtype=np.float64).reshape(ym.shape[:-1], order="F")
    gx, glam = np.empty(ym.shape), np.empty(ym.shape[:-1])
    for idx in np.ndindex(*ym.shape[:-1]):
        gx[idx], glam[idx] = vjp_1d(ym[idx], mum[idx], gm[idx], lam)
    return np.moveaxis(gx, -1, dim), glam.ravel(order="F")


def cond(n, mu):
    """cond(T + mu I) from the eigenvalues 4 sin^2(k pi / 2n), k = 1 .. n-1, of T."""
    return (4.0 + mu) / (mu + 4.0 * np.sin(np.pi / (2.0 * n)) ** 2)


def bar(n, mu, g):
    """The bound on |device - model|: 64 n ulps of the largest cotangent entry, amplified by the solve's condition number."""
    return 64.0 * n * 2.0 ** -52 * float(np.max(cond(n, np.asarray(mu, dtype=np.float64)))) * float(np.max(np.abs(g)))


def cases(seed=SEED, lengths=LENGTHS, lambdas=LAMBDAS):
    """(n, lambda, x, c, o): unit-normal signal, cotangent and a second cotangent (for the symmetry check)."""
    rng = np.random.default_rng(seed)
    for n in lengths:
        for lam in lambdas:
            yield n, lam, rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
