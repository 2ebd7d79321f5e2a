"""The numpy model of the Douglas-Rachford and Dykstra derivatives with a norm per term (tests/tvp_vjp_model.py) against central
differences (h = 1e-5) of the same recurrences built from the CPU oracle's exact TV-L1 and TV-L2 proxes: within 1e-7, the bar of a
composed loop's backward.  No GPU.  The model is the yardstick of tests/test_gpu_tvp_vjp.py.

Inputs are chosen (seeds, penalties, the scaling of the slices) so that the derivative is well defined in every sweep of every case, and
the tests assert it: every TV-L2 fibre stays 20 % away from its kink ||T^-1 D x|| = lambda, no jump of a TV-L1 sweep output lies where
the step rule would have to decide, and every case holds TV-L2 fibres inside the ball (mu = 0) as well as active ones."""
import numpy as np
import pytest

import tvp_vjp_model as tp
import vjp_model as vm

# (seed, shape, (W1, W2), (p_col, p_row), maxit, amps, axis): tp.draw_rows(seed, shape, amps, axis)
DR_CASES = ((1, (9, 7), (0.3, 0.25), (1, 2), 4, (3.0, 0.02), 0),
            (1, (9, 7), (0.3, 0.25), (2, 1), 4, (3.0, 0.02), 1),
            (3, (9, 7), (0.3, 0.25), (2, 2), 4, (3.0, 0.02), 0))
# (seed, loop, shape, dims, lambda_0, ps, iters, amps, axis): lambda_i = lambda_0 (1 + 0.2 i), as the C entry point receives them
PD_CASES = ((17, "pd2", (9, 7), (1, 2), 0.4, (1, 2), 3, (3.0, 0.02), 0),
            (1, "pd2", (9, 7), (1, 2), 0.2, (2, 1), 3, (3.0, 0.02), 1),
            (1, "pd2", (9, 7), (1, 2), 0.2, (2, 2), 3, (3.0, 0.02), 1),
            (1, "pd2", (9, 7), (2,), 0.2, (2,), 3, (3.0, 0.02), 0),
            (6, "pd", (6, 5, 4), (1, 2, 3), 0.4, (2, 1, 1), 3, (2.0, 0.05, 2.0), 2),
            (2, "pd", (6, 5, 4), (1, 2, 3), 0.2, (1, 2, 2), 3, (3.0, 0.02), 1),
            (5, "pd", (6, 5, 4), (1, 2, 1, 3), 0.4, (1, 1, 2, 1), 3, (2.0, 0.05, 2.0), 1))   # two terms share dimension 1, one of them TV-L2


def lams_of(lam0, count):
    return tuple(lam0 * (1 + 0.2 * i) for i in range(count))


def check(tape, loss, x, pens, gx, glam, name):
    """The conditions on the inputs, then gx and glam against central differences of loss(x, pens)."""
    tp.assert_well_defined(tape)
    inside, active = tp.branches(tape)
    assert inside > 0 and active > 0, (name, inside, active)
    fd = vm.central_x(lambda v: loss(v, pens), np.ascontiguousarray(x.copy()), tp.FD_H)
    ex = float(np.max(np.abs(fd - gx)))
    el = 0.0
    for i in range(len(pens)):
        up, dn = list(pens), list(pens)
        up[i] += tp.FD_H
        dn[i] -= tp.FD_H
        el = max(el, abs((loss(x, up) - loss(x, dn)) / (2 * tp.FD_H) - glam[i]))
    print(f"{name}: |gx - fd| {ex:.2e}, |glam - fd| {el:.2e} (bar {tp.FD_TOL:.0e}); TV-L2 fibres inside {inside}, active {active}, "
          f"clearance {tp.kink_clearance(tape):.2f}, worst cond {tp.worst_cond(tape):.1f}")
    assert ex <= tp.FD_TOL and el <= tp.FD_TOL, name


@pytest.mark.parametrize("seed,shape,W,ps,maxit,amps,axis", DR_CASES)
def test_dr_model_equals_central_differences(oracle, seed, shape, W, ps, maxit, amps, axis):
    U, g = tp.draw_rows(seed, shape, amps, axis)
    out, tape = tp.dr_forward(oracle, U, W[0], W[1], ps[0], ps[1], maxit)
    gU, glam, sweeps, _ = tp.dr_reverse(tape, g)
    assert sweeps == 2 * maxit + 2
    loss = lambda u, w: float(np.sum(g * tp.dr_forward(oracle, u, w[0], w[1], ps[0], ps[1], maxit)[0]))   # noqa: E731
    check(tape, loss, U, W, gU, glam, f"dr {shape} p {ps}")


@pytest.mark.parametrize("seed,loop,shape,dims,lam0,ps,iters,amps,axis", PD_CASES)
def test_pd_model_equals_central_differences(oracle, seed, loop, shape, dims, lam0, ps, iters, amps, axis):
    y, g = tp.draw_rows(seed, shape, amps, axis)
    lams = lams_of(lam0, len(dims))
    out, tape = tp.pd_forward(oracle, loop, y, lams, dims, ps, iters)
    gy, glam, _, _ = tp.pd_reverse(loop, tape, g)
    loss = lambda u, w: float(np.sum(g * tp.pd_forward(oracle, loop, u, w, dims, ps, iters)[0]))   # noqa: E731
    check(tape, loss, y, lams, gy, glam, f"{loop} {shape} dims {dims} p {ps}")


def test_all_norms_one_is_the_l1_model(oracle):
    """With every norm 1 the model is dr_vjp_model's / pd_vjp_model's, bit for bit."""
    import dr_vjp_model as dm
    import pd_vjp_model as pm
    U, g, _, _ = dm.draw(1, (9, 7), 0.3)
    out, tape = tp.dr_forward(oracle, U, 0.3, 0.21, 1, 1, 3)
    out0, tape0 = dm.forward(oracle, U, 0.3, 0.21, 3)
    gU, glam, _, _ = tp.dr_reverse(tape, g)
    gU0, gW1, gW2 = dm.reverse(tape0, g)
    assert np.array_equal(out, out0) and np.array_equal(gU, gU0)
    assert np.allclose(glam, [gW1.sum(), gW2.sum()], rtol=0, atol=1e-13)
    for loop, dims, lams in (("pd", (1, 2, 1), (0.3, 0.2, 0.12)), ("pd2", (1, 2), (0.25, 0.4))):
        y, g = pm.draw(2, (12, 10))
        out, tape = tp.pd_forward(oracle, loop, y, lams, dims, (1,) * len(dims), 4)
        out0, tape0 = pm.forward(oracle, loop, y, lams, dims, 4)
        gy, glam, sweeps, A = tp.pd_reverse(loop, tape, g)
        gy0, glam0, sweeps0, A0 = pm.reverse(loop, tape0, g, dims)
        assert np.array_equal(out, out0) and np.array_equal(gy, gy0) and np.array_equal(glam, glam0) and (sweeps, A) == (sweeps0, A0)
        assert tp.bar(tape, sweeps, A) == pm.bar((12, 10), dims, sweeps, A)
