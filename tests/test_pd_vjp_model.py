"""The derivative of the two Dykstra loops behind tvgen without a GPU: the reverse recurrences of tests/pd_vjp_model.py against central
differences (h = 1e-5) of the model's own forward, which is built on the CPU oracle's 1-D prox.  The model is the yardstick of
tests/test_gpu_pd_vjp.py; this is what it rests on.  The iteration count is fixed at 6, the data are unit noise and every penalty is
at least 0.05: no perturbation changes a step pattern, and there is no stopping rule to change the count."""
import numpy as np
import pytest

import pd_vjp_model as pm
import vjp_model as vm


@pytest.mark.parametrize("seed,loop,shape,dims,lams", pm.CASES)
def test_reverse_against_central_differences(oracle, seed, loop, shape, dims, lams):
    y, g = pm.draw(seed, shape)
    assert min(lams) >= 0.05
    out, tape = pm.forward(oracle, loop, y, lams, dims, pm.ITERS)
    assert len(tape) == (1 if loop == "pd2" and len(lams) == 1 else pm.ITERS)
    pm.assert_tape_unambiguous(tape, dims)
    gy, glam, sweeps, A = pm.reverse(loop, tape, g, dims)
    assert sweeps == len(tape) * len(lams) and glam.shape == (len(lams),) and A >= np.linalg.norm(g)

    def loss(u, ls=lams):
        return float(np.sum(g * pm.forward(oracle, loop, u, ls, dims, pm.ITERS)[0]))

    h = vm.FD_H
    ex = float(np.max(np.abs(vm.central_x(loss, y.copy()) - gy)))
    el = 0.0
    for i in range(len(lams)):
        up, dn = list(lams), list(lams)
        up[i] += h
        dn[i] -= h
        el = max(el, abs((loss(y, up) - loss(y, dn)) / (2 * h) - glam[i]))
    print(f"seed {seed} {loop} {shape} dims {dims}: |gy - fd| {ex:.2e}, |glam - fd| {el:.2e}, A / |g| {A / np.linalg.norm(g):.2f}")
    assert ex <= vm.FD_TOL and el <= vm.FD_TOL


def test_one_term_of_the_two_term_loop_is_one_sweep(oracle):
    """x + p stays y when there is one term: any iteration count gives the single sweep and its derivative."""
    y, g = pm.draw(6, (12, 10))
    out, tape = pm.forward(oracle, "pd2", y, (0.35,), (1,), 4)
    assert len(tape) == 1 and np.array_equal(out, pm.prox(oracle, y, 0, 0.35))
    gy, glam, sweeps, _ = pm.reverse("pd2", tape, g, (1,))
    want, gw, _ = vm.vjp_nd(out, g, 0)
    assert sweeps == 1 and np.array_equal(gy, want) and glam[0] == gw.sum()
