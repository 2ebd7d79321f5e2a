"""The numpy model of the Douglas-Rachford and Dykstra derivatives with general-p terms (tests/tvpg_vjp_model.py), without a
GPU: (1) adjointness -- <g, T v> = <T' g, v> against the forward-mode linearisation of the same recurrence, to rounding, which does not
go through the inexact forward; (2) central differences (h = 1e-5) of the recurrence built from the CPU oracle's exact p = 1 / p = 2
proxes and the host build of tvpcore.hpp (tests/tvp_host.cpp) for a general p, within gm.FD_BAR: four times the worst figure measured
on these very cases.  The model is the yardstick behind tests/test_gpu_tvpg_vjp.py.

Inputs are unit-normal, penalties 0.05 and 0.8.  No case is skipped: the last test counts them."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import tvpg_vjp_model as gm
import vjp_model as vm

HERE = os.path.dirname(os.path.abspath(__file__))
LAMBDAS = (0.05, 0.8)
ITERS = 3
DR_CASES = tuple(((9, 7), ps, lam) for ps in ((1.5, 1), (3, 1.5), (2, 3)) for lam in LAMBDAS)
# (loop, shape, dims, ps)
PD_CASES = tuple(case + (lam,) for case in (("pd2", (9, 7), (1, 2), (1.5, 3)), ("pd2", (9, 7), (2,), (1.5,)), ("pd", (5, 6, 4), (1, 2, 3), (1, 3, 1.5)))
                 for lam in LAMBDAS)
RAN = set()


@pytest.fixture(scope="module")
def prox(oracle):
    out = os.path.join(tempfile.mkdtemp(prefix="ptv_tvpg_"), "libtvp_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "tvp_host.cpp")], check=True)
    lib = C.CDLL(out)
    lib.host_tvp_fibre.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.host_tvp_fibre.restype = C.c_int

    def forward(y, lam, p):
        x = np.full(y.size, np.nan)
        assert not lib.host_tvp_fibre(y.ctypes.data, x.ctypes.data, y.size, float(lam), float(p), None, None, None)
        return x

    return gm.make_prox(oracle, forward)


def draw(shape, ps, lam):
    rng = np.random.default_rng(700 + int(10 * sum(ps)) + int(100 * lam) + sum(shape))
    return rng.standard_normal(shape), rng.standard_normal(shape), rng.standard_normal(shape)


def lams_of(lam, count):
    return tuple(lam * (1 + 0.2 * i) for i in range(count))


def check(name, tape, loss, x, pens, g, v, gx, glam, tangent):
    # (1) adjointness
    lhs, rhs = float(np.sum(g * tangent)), float(np.sum(gx * v))
    adj = abs(lhs - rhs) / (np.linalg.norm(g) * np.linalg.norm(v))
    # (2) central differences
    fd = vm.central_x(lambda u: loss(u, pens), np.ascontiguousarray(x.copy()), gm.FD_H)
    ex = float(np.max(np.abs(np.asarray(fd).reshape(x.shape) - gx)))
    el = 0.0
    for i in range(len(pens)):
        up, dn = list(pens), list(pens)
        up[i] += gm.FD_H
        dn[i] -= gm.FD_H
        el = max(el, abs((loss(x, up) - loss(x, dn)) / (2 * gm.FD_H) - glam[i]))
    mean, iterative = gm.branches(tape)
    print(f"{name}: adjointness {adj:.2e}, |gx - fd| {ex:.2e}, |glam - fd| {el:.2e} (bar {gm.FD_BAR:.1e}); general-p fibres: mean {mean}, "
          f"iterative {iterative}")
    RAN.add(name)
    assert adj <= gm.ADJOINT_TOL, name
    assert ex <= gm.FD_BAR and el <= gm.FD_BAR, name


@pytest.mark.parametrize("shape,ps,lam", DR_CASES)
def test_dr_model(prox, shape, ps, lam):
    U, g, v = draw(shape, ps, lam)
    W = (lam, 1.2 * lam)
    out, tape = gm.dr_forward(prox, U, W[0], W[1], ps[0], ps[1], ITERS)
    gU, glam = gm.dr_reverse(tape, g)
    loss = lambda u, w: float(np.sum(g * gm.dr_forward(prox, u, w[0], w[1], ps[0], ps[1], ITERS)[0]))   # noqa: E731
    check(f"dr {shape} p {ps} lambda {lam}", tape, loss, U, W, g, v, gU, glam, gm.dr_tangent(tape, v))


@pytest.mark.parametrize("loop,shape,dims,ps,lam", PD_CASES)
def test_pd_model(prox, loop, shape, dims, ps, lam):
    y, g, v = draw(shape, ps, lam)
    lams = lams_of(lam, len(dims))
    out, tape = gm.pd_forward(prox, loop, y, lams, dims, ps, ITERS)
    gy, glam = gm.pd_reverse(loop, tape, g)
    loss = lambda u, w: float(np.sum(g * gm.pd_forward(prox, loop, u, w, dims, ps, ITERS)[0]))   # noqa: E731
    check(f"{loop} {shape} dims {dims} p {ps} lambda {lam}", tape, loss, y, lams, g, v, gy, glam, gm.pd_tangent(loop, tape, v))


def test_norms_in_one_two_are_the_existing_model(oracle):
    """With every norm in {1, 2} the model is tvp_vjp_model's, bit for bit."""
    import tvp_vjp_model as tp
    prox = gm.make_prox(oracle, None)
    U, g = tp.draw_rows(1, (9, 7), (3.0, 0.02), 0)
    out, tape = gm.dr_forward(prox, U, 0.3, 0.25, 1, 2, 3)
    out0, tape0 = tp.dr_forward(oracle, U, 0.3, 0.25, 1, 2, 3)
    assert np.array_equal(out, out0)
    assert all(np.array_equal(a, b) for a, b in zip(gm.dr_reverse(tape, g), tp.dr_reverse(tape0, g)[:2]))
    for loop, dims, ps in (("pd2", (1, 2), (2, 1)), ("pd", (1, 2, 1), (1, 2, 2))):
        lams = lams_of(0.2, len(dims))
        out, tape = gm.pd_forward(prox, loop, U, lams, dims, ps, 3)
        out0, tape0 = tp.pd_forward(oracle, loop, U, lams, dims, ps, 3)
        assert np.array_equal(out, out0)
        assert all(np.array_equal(a, b) for a, b in zip(gm.pd_reverse(loop, tape, g), tp.pd_reverse(loop, tape0, g)[:2]))


def test_no_case_was_skipped():
    """Runs last in this file: every case above went through both checks."""
    assert len(RAN) == len(DR_CASES) + len(PD_CASES), sorted(RAN)
