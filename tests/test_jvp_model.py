"""The forward-mode derivatives without a GPU: the numpy models of tests/jvp_model.py against central differences (h = 1e-5) of their own
forward, which is built on the CPU oracle's 1-D prox, and against the reverse-mode models (tests/vjp_model.py, tests/dr_vjp_model.py) by
the adjoint identity  <g, dy> = <gx, dx> + <gw, dr>.  The models are the yardsticks of tests/test_jvp_host.py and of the GPU tests; this is
what they rest on.

Inputs: unit Gaussian signals, lambda in {0.1, 0.5}, per-edge weights U(0.05, 0.5).  Tangents are scaled to a largest entry of 1, so that
a displaced forward moves no sample by more than h; every case asserts that no jump of the prox outputs lies within 1e-6 of the step
rule's threshold region, so the two displaced solves share their segmentation (no seed of this file had to be replaced for that)."""
import numpy as np
import pytest

import dr_vjp_model as dm
import jvp_model as jm
import vjp_model as vm

H, BAR = vm.FD_H, vm.FD_TOL
LENGTHS = (1, 2, 15, 16, 17, 33, 129)
LAMBDAS = (0.1, 0.5)


def unit(a):
    m = float(np.max(np.abs(a))) if a.size else 0.0
    return a / m if m > 0 else a


def fibre_case(n, lam, weighted, seed):
    rng = np.random.default_rng(seed)
    x, dx, g = rng.standard_normal(n), unit(rng.standard_normal(n)), rng.standard_normal(n)
    w = rng.uniform(0.05, 0.5, max(n - 1, 0)) if weighted else np.full(max(n - 1, 0), lam)
    dr = unit(rng.uniform(-1.0, 1.0, max(n - 1, 0)))
    return x, dx, g, w, dr


def fibre_prox(oracle, x, w):
    return x.copy() if x.size == 1 else oracle.tv1_weighted(x, w)


@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("lam", LAMBDAS)
def test_fibre_model_against_central_differences_and_the_vjp(oracle, lam, weighted):
    worst = worst_adj = 0.0
    for n in LENGTHS:
        x, dx, g, w, dr = fibre_case(n, lam, weighted, 100 * n + int(10 * lam) + weighted)
        y = fibre_prox(oracle, x, w)
        vm.assert_unambiguous(y)
        ones = np.ones(max(n - 1, 0))
        zero_x, zero_r = np.zeros(n), np.zeros(max(n - 1, 0))
        for name, ddx, ddr in (("dx", dx, zero_r), ("dlam", zero_x, ones), ("dr", zero_x, dr), ("all", dx, dr + 0.5 * ones)):
            dy, _ = jm.jvp_1d(y, ddx, ddr)
            fd = (fibre_prox(oracle, x + H * ddx, w + H * ddr) - fibre_prox(oracle, x - H * ddx, w - H * ddr)) / (2 * H)
            err = float(np.max(np.abs(fd - dy)))
            worst = max(worst, err)
            assert err <= BAR, (n, lam, weighted, name, err)
            gx, gw, _ = vm.vjp_1d(y, g)
            adj = abs(float(np.dot(g, dy)) - float(np.dot(gx, ddx)) - float(np.dot(gw, ddr)))
            # both sides are sums of n products of segment means: the certifier's rounding rule on each, times the other vector's norm
            bound = 2 * vm.rounding_bound(n, g) * (np.linalg.norm(ddx) + np.linalg.norm(ddr) + 1.0)
            worst_adj = max(worst_adj, adj)
            assert adj <= bound, (n, lam, weighted, name, adj, bound)
    print(f"fibre model lambda {lam} weighted {weighted}: worst |fd - dy| {worst:.2e} (bar {BAR:.0e}), worst adjoint defect {worst_adj:.2e}")


def test_an_uniform_tangent_is_a_constant_per_edge_tangent_and_zero_stays_zero(oracle):
    rng = np.random.default_rng(5)
    x = rng.standard_normal(60)
    y = oracle.tv1_linearized(x, 0.3)
    assert np.array_equal(jm.jvp_1d(y, np.zeros(60), np.zeros(59))[0], np.zeros(60))
    dy, v = jm.jvp_1d(y, np.zeros(60), np.full(59, 2.0))
    assert abs(v.sum()) <= 1e-12          # E telescopes: the mean of the prox does not depend on the penalties
    assert np.any(dy != 0.0)


DR_CASES = ((21, (9, 7), 0.1, 35, False), (22, (12, 5), 0.5, 35, False), (23, (1, 9), 0.5, 35, False), (24, (8, 1), 0.1, 35, False),
            (25, (9, 7), 0.5, 1, False), (26, (9, 7), 0.1, 35, True), (27, (12, 5), 0.5, 10, True))


@pytest.mark.parametrize("seed,shape,lam,maxit,weighted", DR_CASES)
def test_dr_model_against_central_differences_and_the_vjp(oracle, seed, shape, lam, maxit, weighted):
    rng = np.random.default_rng(seed)
    U, dU, g = rng.standard_normal(shape), unit(rng.standard_normal(shape)), rng.standard_normal(shape)
    s1, s2 = jm.edge_shapes(shape)
    W1m = rng.uniform(0.05, 0.5, s1) if weighted else np.full(s1, lam)
    W2m = rng.uniform(0.05, 0.5, s2) if weighted else np.full(s2, 0.7 * lam)
    dW1, dW2 = unit(rng.uniform(-1.0, 1.0, s1)), unit(rng.uniform(-1.0, 1.0, s2))

    def forward(u, w1, w2):
        return dm.forward(oracle, u, 0.0, 0.0, maxit, w1, w2)

    out, tape = forward(U, W1m, W2m)
    dm.assert_tape_unambiguous(tape)
    gU, gW1, gW2 = dm.reverse(tape, g)
    z, z1, z2 = np.zeros(shape), np.zeros(s1), np.zeros(s2)
    worst = 0.0
    for name, a, b, c in (("dU", dU, z1, z2), ("dlam_col", z, np.ones(s1), z2), ("dlam_row", z, z1, np.ones(s2)), ("maps", z, dW1, dW2),
                          ("all", dU, dW1 + 0.5, dW2 - 0.25)):
        ds, entering = jm.dr_jvp(tape, a, b, c)
        fd = (forward(U + H * a, W1m + H * b, W2m + H * c)[0] - forward(U - H * a, W1m - H * b, W2m - H * c)[0]) / (2 * H)
        err = float(np.max(np.abs(fd - ds)))
        worst = max(worst, err)
        assert err <= BAR, (name, err)
        adj = abs(float(np.sum(g * ds)) - float(np.sum(gU * a)) - float(np.sum(gW1 * b)) - float(np.sum(gW2 * c)))
        # (6d's argument: 2 maxit + 2 sweeps, each within the certifier's rounding rule of a non-expansive map, in either mode)
        bound = 2 * dm.sweep_scale(shape, maxit, g) * (np.linalg.norm(a) + np.linalg.norm(b) + np.linalg.norm(c))
        assert adj <= bound, (name, adj, bound)
    print(f"DR model seed {seed} {shape} lambda {lam} maxit {maxit} weighted {weighted}: worst |fd - ds| {worst:.2e} (bar {BAR:.0e})")
