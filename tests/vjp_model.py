"""Plain-numpy model of the derivative of the 1-D TV-L1 prox (what proxtv_tv1_fibres_vjp_dev computes), shared by
tests/test_vjp_host.py and tests/test_gpu_vjp.py.  Not a test module."""
import numpy as np

# the step rule of include/proxtv_amd.h, restated (tests/test_vjp_host.py checks these against the library's header)
STEP_REL = 256.0 * 2.0 ** -52
STEP_ABS = 4e-10

LENGTHS = (1, 2, 3, 7, 63, 64, 65, 127, 129, 300, 1000)
LAMBDAS = (0.05, 0.8, 3.0)
FD_H = 1e-5
FD_TOL = 1e-8


def steps(y):
    y = np.asarray(y, dtype=np.float64)
    return np.abs(np.diff(y)) > STEP_REL * np.maximum(np.abs(y[:-1]), np.abs(y[1:])) + STEP_ABS


def vjp_1d(y, g):
    """(gx, gw, nseg) of one fibre: gx = segment means of g, gw[k] = sign(step k) (gx[k] - gx[k+1]), nseg = trace P."""
    y, g = np.asarray(y, dtype=np.float64), np.asarray(g, dtype=np.float64)
    s = steps(y)
    ids = np.concatenate([[0], np.cumsum(s)]).astype(np.int64)
    gx = (np.bincount(ids, weights=g) / np.bincount(ids))[ids]
    gw = np.where(s, np.sign(np.diff(y)) * (gx[:-1] - gx[1:]), 0.0)
    return gx, gw, int(ids[-1]) + 1


def vjp_nd(y, g, dim):
    """The same along `dim` of an N-D array; nseg in the column-major order of the array with `dim` removed."""
    ym, gm = np.moveaxis(y, dim, -1), np.moveaxis(g, dim, -1)
    gx, gw = np.empty(ym.shape), np.empty(ym.shape[:-1] + (ym.shape[-1] - 1,))
    nseg = np.empty(ym.shape[:-1], dtype=np.int32)
    for idx in np.ndindex(*ym.shape[:-1]):
        gx[idx], gw[idx], nseg[idx] = vjp_1d(ym[idx], gm[idx])
    return np.moveaxis(gx, -1, dim), np.moveaxis(gw, -1, dim), nseg.ravel(order="F")


def assert_unambiguous(y, axis=-1):
    """Precondition of every test: on the prox the model is applied to, no jump lies in (0, 1e-6) -- the step rule has nothing to decide."""
    d = np.abs(np.diff(np.asarray(y, dtype=np.float64), axis=axis))
    assert not np.any((d > 0) & (d < 1e-6)), float(d[(d > 0) & (d < 1e-6)].min())


def rounding_bound(n, g):
    """The certifier's rounding rule for a sum of n terms: 64 n ulps of the largest operand."""
    return 64.0 * n * 2.0 ** -52 * float(np.max(np.abs(g)))


def cases(seed=2026):
    """(n, lambda, x, c, weights) for every length and lambda of the issue: unit Gaussian signal and cotangent, weights lambda U(0.5, 1.5)."""
    rng = np.random.default_rng(seed)
    for n in LENGTHS:
        for lam in LAMBDAS:
            yield n, lam, rng.standard_normal(n), rng.standard_normal(n), lam * rng.uniform(0.5, 1.5, max(n - 1, 0))


def central_x(f, x, h=FD_H):
    """Central differences of the scalar function f in every entry of x."""
    assert x.flags.c_contiguous       # (the entries are perturbed in place through a flat view)
    out = np.empty(x.size)
    flat = x.reshape(-1)
    for i in range(flat.size):
        keep = flat[i]
        flat[i] = keep + h
        up = f(x)
        flat[i] = keep - h
        dn = f(x)
        flat[i] = keep
        out[i] = (up - dn) / (2 * h)
    return out.reshape(x.shape)
