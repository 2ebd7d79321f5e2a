"""Plain-numpy model of the 2-D Douglas-Rachford TV-L1 solve and of its derivative (what proxtv_DR2_TV_vjp_dev computes), shared by
tests/test_dr_vjp_model.py and tests/test_gpu_dr_vjp.py.  Not a test module.

Forward (the unfused recurrence of solvers.hip: dr2_norms), per image, keeping the sweep outputs:
    t = 2 mean(U) ; repeat maxit: x1 = prox_cols(t), x2 = prox_rows(U - t + 2 x1), t <- t - x1 + x2 ;
    x1 = prox_cols(t), out = x2 = prox_rows(U - t + x1)
Reverse: the segmented means P_c / P_r of vjp_model.vjp_nd at those outputs, last sweep first."""
import numpy as np

import vjp_model as vm

MAXIT = 35

# (seed, shape, W1, maxit) of the issue: unit Gaussian U and cotangent, W2 = 0.7 W1
UNIFORM_CASES = ((1, (9, 7), 0.3, 35), (2, (12, 5), 0.8, 35), (4, (1, 9), 0.5, 35), (5, (8, 1), 0.5, 35), (6, (2, 2), 0.4, 35),
                 (7, (20, 20), 1.5, 35), (8, (9, 7), 0.3, 1), (9, (16, 12), 0.6, 10))
# (seed, shape, lambda, maxit): maps lambda U(0.5, 1.5), W1 (M-1, N) then W2 (M, N-1), drawn after U and the cotangent
WEIGHTED_CASES = ((11, (9, 7), 0.3, 35), (12, (12, 5), 0.8, 35))
ROW_RATIO = 0.7


def draw(seed, shape, lam, weighted=False):
    """(U, cotangent, W1m | None, W2m | None) of one case."""
    rng = np.random.default_rng(seed)
    U, g = rng.standard_normal(shape), rng.standard_normal(shape)
    if not weighted:
        return U, g, None, None
    M, N = shape
    return U, g, lam * rng.uniform(0.5, 1.5, (M - 1, N)), lam * rng.uniform(0.5, 1.5, (M, N - 1))


def prox_along(oracle, a, dim, lam, weights=None):
    """The CPU oracle's 1-D prox on every fibre of the 2-D array `a` along `dim`."""
    am = np.moveaxis(a, dim, -1)
    wm = None if weights is None else np.moveaxis(weights, dim, -1)
    out = np.empty(am.shape)
    for idx in np.ndindex(*am.shape[:-1]):
        if am.shape[-1] == 1:
            out[idx] = am[idx]
        else:
            out[idx] = oracle.tv1_linearized(am[idx], lam) if wm is None else oracle.tv1_weighted(am[idx], wm[idx])
    return np.moveaxis(out, -1, dim)


def forward(oracle, U, W1, W2, maxit=MAXIT, W1m=None, W2m=None):
    """(out, tape): tape[k] = (x1_k, x2_k) for k = 0 .. maxit, the last pair being the final sweeps'."""
    U = np.asarray(U, dtype=np.float64)
    cols = lambda a: prox_along(oracle, a, 0, W1, W1m)   # noqa: E731
    rows = lambda a: prox_along(oracle, a, 1, W2, W2m)   # noqa: E731
    t = np.full(U.shape, 2.0 * U.mean())
    tape = []
    for _ in range(maxit):
        x1 = cols(t)
        x2 = rows(U - (t - 2.0 * x1))
        tape.append((x1, x2))
        t = t - x1 + x2
    x1 = cols(t)
    x2 = rows(U - (t - x1))
    tape.append((x1, x2))
    return x2, tape


def reverse(tape, g):
    """(gU, gW1, gW2) for the cotangent g of `out`: gW1 (M-1, N) and gW2 (M, N-1) are per edge, their sums the gradients in uniform
    penalties."""
    x1, x2 = tape[-1]
    a, gW2, _ = vm.vjp_nd(x2, g, 1)
    gU = a.copy()
    d, gW1, _ = vm.vjp_nd(x1, a, 0)
    gbar = d - a
    for x1, x2 in reversed(tape[:-1]):
        a, w2, _ = vm.vjp_nd(x2, gbar, 1)
        gU += a
        gW2 = gW2 + w2
        c = 2.0 * a - gbar
        d, w1, _ = vm.vjp_nd(x1, c, 0)
        gW1 = gW1 + w1
        gbar = gbar - a + d
    gU += 2.0 * gbar.sum() / gbar.size        # t0 = 2 mean(U)
    return gU, gW1, gW2


def compose(torch, autograd, U, W1, W2, maxit=MAXIT, W1m=None, W2m=None):
    """The same recurrence written the way a user had to before the native derivative: autograd.tv1_fibres and torch's pointwise
    operations on CUDA tensors, 2 (maxit + 1) prox nodes in a torch graph.  Differentiable in U, in 0-d tensors W1 / W2 and in the maps."""
    t = 2.0 * U.mean() * torch.ones_like(U)
    for _ in range(maxit):
        x1 = autograd.tv1_fibres(t, W1, 0, weights=W1m)
        x2 = autograd.tv1_fibres(U - (t - 2.0 * x1), W2, 1, weights=W2m)
        t = t - x1 + x2
    x1 = autograd.tv1_fibres(t, W1, 0, weights=W1m)
    return autograd.tv1_fibres(U - (t - x1), W2, 1, weights=W2m)


def assert_tape_unambiguous(tape):
    """Precondition of every test: no jump of any taped prox output lies in [1e-12, 1e-6] -- the step rule has nothing to decide.  (Jumps
    below 1e-12 are rounding inside a segment: the oracle leaves some of 4e-16 on larger images.)"""
    for k, (x1, x2) in enumerate(tape):
        for name, y, axis in (("x1", x1, 0), ("x2", x2, 1)):
            d = np.abs(np.diff(y, axis=axis))
            bad = (d >= 1e-12) & (d <= 1e-6)
            assert not np.any(bad), (k, name, float(d[bad].min()))


def sweep_scale(shape, maxit, g):
    """The bar of the device tests: the certifier's rounding rule per sum (64 n ulps), times the 2 maxit + 2 accumulated sweeps, with
    every intermediate cotangent bounded by ||g||_2 (the per-iteration map is averaged, hence non-expansive)."""
    return 64.0 * (2 * maxit + 2) * max(shape[0], shape[1]) * 2.0 ** -52 * float(np.linalg.norm(g))
