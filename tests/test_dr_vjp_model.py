"""The derivative of the 2-D Douglas-Rachford TV-L1 solve without a GPU: the reverse recurrence of tests/dr_vjp_model.py against
central differences (h = 1e-5) of its own forward, which is built on the CPU oracle's 1-D prox.  The model is the yardstick of
tests/test_gpu_dr_vjp.py; this is what it rests on."""
import numpy as np
import pytest

import dr_vjp_model as dm
import vjp_model as vm


@pytest.mark.parametrize("seed,shape,W1,maxit", dm.UNIFORM_CASES)
def test_uniform_penalties(oracle, seed, shape, W1, maxit):
    U, g, _, _ = dm.draw(seed, shape, W1)
    W2 = dm.ROW_RATIO * W1
    out, tape = dm.forward(oracle, U, W1, W2, maxit)
    assert len(tape) == maxit + 1 and out is tape[-1][1]
    dm.assert_tape_unambiguous(tape)
    gU, gW1, gW2 = dm.reverse(tape, g)
    assert gW1.shape == (shape[0] - 1, shape[1]) and gW2.shape == (shape[0], shape[1] - 1)

    def loss(u, w1=W1, w2=W2):
        return float(np.sum(g * dm.forward(oracle, u, w1, w2, maxit)[0]))

    h = vm.FD_H
    ex = float(np.max(np.abs(vm.central_x(loss, U.copy()) - gU)))
    e1 = abs((loss(U, w1=W1 + h) - loss(U, w1=W1 - h)) / (2 * h) - gW1.sum())
    e2 = abs((loss(U, w2=W2 + h) - loss(U, w2=W2 - h)) / (2 * h) - gW2.sum())
    print(f"seed {seed} {shape} W1 {W1} maxit {maxit}: |gU - fd| {ex:.2e}, |dW1 - fd| {e1:.2e}, |dW2 - fd| {e2:.2e}")
    assert ex <= vm.FD_TOL and e1 <= vm.FD_TOL and e2 <= vm.FD_TOL


@pytest.mark.parametrize("seed,shape,lam,maxit", dm.WEIGHTED_CASES)
def test_weight_maps(oracle, seed, shape, lam, maxit):
    U, g, W1m, W2m = dm.draw(seed, shape, lam, weighted=True)
    out, tape = dm.forward(oracle, U, 0.0, 0.0, maxit, W1m, W2m)
    dm.assert_tape_unambiguous(tape)
    gU, gW1, gW2 = dm.reverse(tape, g)

    def loss(u, w1=W1m, w2=W2m):
        return float(np.sum(g * dm.forward(oracle, u, 0.0, 0.0, maxit, w1, w2)[0]))

    ex = float(np.max(np.abs(vm.central_x(loss, U.copy()) - gU)))
    e1 = float(np.max(np.abs(vm.central_x(lambda w: loss(U, w1=w), W1m.copy()) - gW1)))
    e2 = float(np.max(np.abs(vm.central_x(lambda w: loss(U, w2=w), W2m.copy()) - gW2)))
    print(f"seed {seed} {shape} lambda {lam}: |gU - fd| {ex:.2e}, |gW1 - fd| {e1:.2e}, |gW2 - fd| {e2:.2e}")
    assert ex <= vm.FD_TOL and e1 <= vm.FD_TOL and e2 <= vm.FD_TOL
