"""Plain-numpy dense model of the derivative of the general-p TV-Lp fibre prox (what proxtv_tvpg_fibres_vjp_dev computes),
shared by tests/test_tvp_vjp_host.py and tests/test_gpu_tvp_fibres_vjp.py.  Not a test module.

Per fibre of n samples: D the (n-1) x n difference matrix, T = D D', x = prox(y) the forward's OUTPUT, w = D x, N = ||w||_p,
s = |w| / N, q = p / (p - 1), phi = sign(w) s^(p-1) (the gradient of ||.||_p at w), g the cotangent.
    J = (I + lambda D' H D)^-1 ,  H = (p-1)/N (diag s^(p-2) - phi phi')     symmetric: the VJP is the JVP
    p > 2 (primal arm)   M = I + lambda D' diag((p-1)/N s^(p-2)) D, b = D' phi, c = lambda (p-1) / N, a = M^-1 g, e = M^-1 b,
                         gx = a + c (b'a) / (1 - c b'e) e
    p < 2 (dual arm)     H = T + diag((q-1) N / lambda s^(2-p)), h = D g, a = H^-1 h, e = H^-1 w, gx = g - D'(a - (w'a) / (w'e) e)
    both                 glam = -gx' D' phi
    n == 1 or lambda <= 0: gx = g ;  x constant (N == 0 exactly): gx = mean(g) ;  glam = 0 in all of them
"""
import numpy as np

LENGTHS = (1, 2, 3, 7, 8, 9, 16, 17, 64, 65, 129)     # (the kernel handles 8 samples per step)
PS = (1.1, 1.5, 1.9, 3.0, 7.0, 20.0)
LAMBDAS = (0.05, 0.8, 3.0, 40.0)
SEED = 41
FD_H = 1e-5
# |model - central differences (h = 1e-5) of the forward| over gx and glam: four times the largest figure of each arm on the grid above
# with the host-built forward (dual 6.3e-6 at n = 2, p = 1.1, lambda = 0.05; primal 8.7e-5 at n = 8, p = 20, lambda = 3).
# The figures do not move with h (1e-4 .. 1e-6): they are the derivative of the forward's own stopping error (it stops at a duality gap
# of 1e-8, wherever its last Newton step landed), not the truncation or the rounding of the differences
FD_BAR = {"dual": 4 * 6.3e-6, "primal": 4 * 8.7e-5}


def arm(p):
    return "primal" if p > 2 else "dual"


def dmat(n):
    return np.diff(np.eye(n), axis=0)


def parts(x, p):
    """(w, N, s, phi) of the output x; N is summed in powers of |w| / max|w| like the kernel's (no overflow for p up to 100)."""
    w = np.diff(np.asarray(x, dtype=np.float64))
    wmax = float(np.max(np.abs(w))) if w.size else 0.0
    if not wmax > 0:
        return w, 0.0, np.zeros_like(w), np.zeros_like(w)
    N = wmax * float(np.sum((np.abs(w) / wmax) ** p)) ** (1.0 / p)
    s = np.abs(w) / N
    return w, N, s, np.sign(w) * s ** (p - 1.0)


def system(x, lam, p):
    """The arm's matrix and the amplification of its rank-one correction: (K, amp) -- amp = 1 / (1 - c b'e) for p > 2,
    ||w||^2 / (w'e) for p < 2."""
    n = len(x)
    w, N, s, phi = parts(x, p)
    D = dmat(n)
    if p > 2:
        K = np.eye(n) + lam * D.T @ np.diag((p - 1.0) / N * s ** (p - 2.0)) @ D
        b, c = D.T @ phi, lam * (p - 1.0) / N
        return K, 1.0 / (1.0 - c * float(b @ np.linalg.solve(K, b)))
    q = p / (p - 1.0)
    K = D @ D.T + np.diag((q - 1.0) * N / lam * s ** (2.0 - p))
    return K, float(w @ w) / float(w @ np.linalg.solve(K, w))


def vjp_1d(x, g, lam, p):
    """(gx, glam) of one fibre from the prox's output x."""
    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    n = x.size
    if n < 2 or not lam > 0:
        return g.copy(), 0.0
    w, N, s, phi = parts(x, p)
    if N == 0.0:
        return np.full(n, g.mean()), 0.0
    D = dmat(n)
    K, _ = system(x, lam, p)
    if p > 2:
        b, c = D.T @ phi, lam * (p - 1.0) / N
        a, e = np.linalg.solve(K, g), np.linalg.solve(K, b)
        gx = a + c * float(b @ a) / (1.0 - c * float(b @ e)) * e
    else:
        a, e = np.linalg.solve(K, D @ g), np.linalg.solve(K, w)
        gx = g - D.T @ (a - float(w @ a) / float(w @ e) * e)
    return gx, -float(gx @ (D.T @ phi))


def vjp_nd(x, g, lam, p, dim):
    """The same along `dim` of an N-D array; the returned glam in the column-major order of the array with `dim` removed."""
    xm, gm = np.moveaxis(x, dim, -1), np.moveaxis(g, dim, -1)
    gx, glam = np.empty(xm.shape), np.empty(xm.shape[:-1])
    for idx in np.ndindex(*xm.shape[:-1]):
        gx[idx], glam[idx] = vjp_1d(xm[idx], gm[idx], lam, p)
    return np.moveaxis(gx, -1, dim), glam.ravel(order="F")


def bar(x, g, lam, p):
    """The bound on |core - model| (and |device - model|): 64 n ulps of the largest cotangent entry, amplified by the condition number of
    the arm's matrix and by its rank-one correction (tv2_vjp_model.bar's form)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    if n < 2 or not lam > 0 or parts(x, p)[1] == 0.0:
        return 64.0 * n * 2.0 ** -52 * float(np.max(np.abs(g)))
    K, amp = system(x, lam, p)
    return 64.0 * n * 2.0 ** -52 * float(np.linalg.cond(K)) * amp * float(np.max(np.abs(g)))


def cases(seed=SEED, lengths=LENGTHS, ps=PS, lambdas=LAMBDAS):
    """(n, p, lambda, y, g, o): unit-normal signal, cotangent and a second cotangent (for the symmetry check)."""
    rng = np.random.default_rng(seed)
    for n in lengths:
        for p in ps:
            for lam in lambdas:
                yield n, p, lam, rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
