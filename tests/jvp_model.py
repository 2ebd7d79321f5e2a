"""Plain-numpy models of the forward-mode derivatives (what proxtv_tv1_fibres_jvp_dev and proxtv_DR2_TV_jvp_dev compute),
shared by tests/test_jvp_model.py, tests/test_jvp_host.py and the GPU tests.  Not a test module.

Fibre: dy = P (dx + E(sigma, dr)), E[i] = sigma_i dr_i - sigma_{i-1} dr_{i-1}, with P and the step rule of tests/vjp_model.py.
Douglas-Rachford: the tangent of the unfused recurrence of tests/dr_vjp_model.py, formed sweep by sweep from the taped outputs."""
import numpy as np

import vjp_model as vm


def inject_1d(y, dr):
    """E(sigma, dr) of one fibre: dr holds one tangent per edge (n - 1 of them)."""
    y = np.asarray(y, dtype=np.float64)
    E = np.zeros(y.size)
    if y.size > 1:
        e = np.where(vm.steps(y), np.sign(np.diff(y)), 0.0) * np.asarray(dr, dtype=np.float64)
        E[:-1] += e
        E[1:] -= e
    return E


def jvp_1d(y, dx, dr):
    """(dy, v) of one fibre: v = dx + E is the vector the segmented mean is applied to."""
    v = np.asarray(dx, dtype=np.float64) + inject_1d(y, dr)
    return vm.vjp_1d(y, v)[0], v


def jvp_nd(y, dx, dr, dim):
    """The same along `dim` of an N-D array; dr has the shape of y with `dim` reduced by one."""
    ym, xm, rm = np.moveaxis(y, dim, -1), np.moveaxis(dx, dim, -1), np.moveaxis(dr, dim, -1)
    dy, v = np.empty(ym.shape), np.empty(ym.shape)
    for idx in np.ndindex(*ym.shape[:-1]):
        dy[idx], v[idx] = jvp_1d(ym[idx], xm[idx], rm[idx])
    return np.moveaxis(dy, -1, dim), np.moveaxis(v, -1, dim)


def dr_jvp(tape, dU, dW1, dW2):
    """(ds, entering) for one image: `tape` is dr_vjp_model.forward's, dW1 (M-1, N) and dW2 (M, N-1) the per-edge penalty tangents (a
    uniform tangent is a constant array).  entering = the sum over all sweeps of the 2-norm of the vector that sweep's segmented mean is
    applied to: what the rounding bound of the device tests is scaled by."""
    dU = np.asarray(dU, dtype=np.float64)
    dt = np.full(dU.shape, 2.0 * dU.mean())
    entering = 0.0
    for k, (x1, x2) in enumerate(tape):
        last = k == len(tape) - 1
        dx1, v1 = jvp_nd(x1, dt, dW1, 0)
        dx2, v2 = jvp_nd(x2, dU - dt + (1.0 if last else 2.0) * dx1, dW2, 1)
        entering += float(np.linalg.norm(v1)) + float(np.linalg.norm(v2))
        if last:
            return dx2, entering
        dt = dt - dx1 + dx2
    raise AssertionError("empty tape")


def edge_shapes(shape):
    M, N = shape[:2]
    return (max(M - 1, 0), N) + tuple(shape[2:]), (M, max(N - 1, 0)) + tuple(shape[2:])
