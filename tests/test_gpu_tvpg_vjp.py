"""The derivatives of the Douglas-Rachford and Dykstra solves with general-p TV-Lp terms on the GPU (option general_p_vjp):
proxtv_DR2_TVp_vjp_dev and proxtv_PD_TVp_vjp_dev through device.dr2_vjp(p_col=, p_row=) / device.tvgen_vjp(ps=), and autograd.tvp_2d /
autograd.tvgen(ps=).

The reference is the same recurrence, with the same iteration count, composed in torch from autograd.tv1_fibres / tv2_fibres /
tvp_fibres (tests/tvpg_vjp_model.py: dr_compose, pd_compose).  The one call and the composition run the same fibre kernels; they differ
in the rounding of the pointwise steps between the sweeps, which feeds an iterative prox that stops at a duality gap of 1e-8.  The bars
are four times the worst difference measured per quantity over the cases of this file (DESIGN.md 6j has the table): COMPOSE_BAR.  The
autograd tests difference the fused device solve itself: FD_BAR, four times the worst measured, the floor being the derivative of the
forward's stopping error as in 6i.

Shapes: (70, 130) (dimension-0 fibres through the transpose, strided rows, more than one wave, lengths no multiple of 8), (65, 3) and
(2, 67) (fibres of 3 and 2 samples, a partial wave), (1, 40) (fibres of one sample; a single dimension-0 fibre), (20, 30, 9) with two
terms sharing a dimension, one fibre of 20000 samples."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import tvpg_vjp_model as gm
import vjp_model as vm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
W = (0.3, 0.25)
NORMS = ((1, 1.5), (1.5, 2), (3, 1.5), (7, 1.1))
DR_CASES = tuple((shape, ps, 2) for shape in ((70, 130), (65, 3), (2, 67), (1, 40)) for ps in NORMS) + (((70, 130), (3, 1.5), 5),)
PD_CASES = tuple(("pd2", (70, 130), (1, 2), ps, 3) for ps in NORMS) + \
    (("pd", (20, 30, 9), (1, 2, 1, 3), (1, 1.5, 3, 1), 3), ("pd", (20, 30, 9), (1, 2, 1, 3), (1.5, 2, 7, 1.1), 2),
     ("pd2", (1, 20000), (2,), (1.5,), 1), ("pd2", (1, 20000), (2,), (3,), 1))
# four times the worst |one call - composition| measured over DR_CASES, PD_CASES and the branch cases: forward result, gradient in x
# (both relative to the largest entry of the reference), penalty gradients (relative to the largest of them).  Measured worst: forward
# 3.07e-15 and penalties 7.34e-15 / 1.07e-14 (DR (2, 67), p = (7, 1.1) / DR (70, 130), p = (1, 1.5)), gx 1.24e-13 (DR (70, 130), p = (7, 1.1))
# -- rounding of the pointwise steps, amplified by the ill-conditioned p = 1.1 / p = 7 fibres; far below the 1e-6 that would be a finding
COMPOSE_BAR = {"forward": 4 * 3.07e-15, "gx": 4 * 1.24e-13, "glam": 4 * 1.07e-14}
# four times the worst |backward - central differences of the fused device solve| measured in the autograd tests: x 1.80e-7 (tvp_2d,
# p = (1.5, 1)), penalties 3.79e-7 (tvgen pd2, p = (1.5, 1)); 6i's 6.7e-8 for one fibre prox is the scale
FD_BAR = {"gx": 4 * 1.80e-7, "glam": 4 * 3.79e-7}


@pytest.fixture(scope="module")
def dev(ptv, clib):
    import torch
    from proxtv_amd import autograd, device

    class Dev:
        pass

    d = Dev()
    d.torch, d.device, d.autograd, d.ptv, d.clib = torch, device, autograd, ptv, clib
    d.up = lambda a: device.to_colmajor(torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda())
    d.down = lambda t: t.cpu().numpy()
    return d


@pytest.fixture
def on(dev):
    """general_p_vjp on for the test, and both switches and the route back to what they were behind it."""
    before = dev.ptv.general_p_vjp(True)
    before_p = dev.ptv.general_p(False)
    dev.ptv.general_p(before_p)
    yield
    dev.ptv.general_p_vjp(before)
    dev.ptv.general_p(before_p)
    dev.clib.proxtv_set_option(b"tvp_vjp_route", 0)


def draw(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape), rng.standard_normal(shape)


def lams_of(loop, dims):
    P = len(dims)
    ws = tuple((0.25 + 0.15 * i) / (P if loop == "pd" else 1) for i in range(P))
    return ws, tuple(w * (P if loop == "pd" else 1) for w in ws)


def dr_call(dev, x, g, ps, maxit, w=W, **kw):
    gx, _, _, glam, y = dev.device.dr2_vjp(dev.up(x), dev.up(g), w[0], w[1], maxit, need_gw="sums", need_y=True, p_col=ps[0], p_row=ps[1], **kw)
    return gx, glam, y


def pd_call(dev, x, g, loop, dims, ps, K, **kw):
    ws, _ = lams_of(loop, dims)
    return dev.device.tvgen_vjp(dev.up(x), dev.up(g), ws, dims, K, loop, need_glam=True, need_y=True, ps=ps, **kw)


def same(a, b, torch):
    return all(torch.equal(u, v) if isinstance(u, torch.Tensor) else np.array_equal(u, v) for u, v in zip(a, b))


@functools.lru_cache(maxsize=None)
def dr_data(shape, ps):
    return draw(shape, 900 + sum(shape) + int(10 * sum(ps)))


@functools.lru_cache(maxsize=None)
def pd_data(shape, ps):
    return draw(shape, 1100 + sum(shape) + int(10 * sum(ps)))


def against(name, dev, got, want):
    """(gx, glam, y) of the one call against (gx, glam, y) of the composition: prints the three figures, then asserts COMPOSE_BAR."""
    (gx, glam, y), (cx, cl, cy) = got, want
    ex = float(np.max(np.abs(dev.down(gx) - cx))) / float(np.max(np.abs(cx)))
    ey = float(np.max(np.abs(dev.down(y) - cy))) / float(np.max(np.abs(cy)))
    el = float(np.max(np.abs(np.asarray(glam) - cl))) / max(float(np.max(np.abs(cl))), 1e-300)
    print(f"COMPOSE {name}: forward {ey:.2e}, gx {ex:.2e}, glam {el:.2e}")
    assert ey <= COMPOSE_BAR["forward"] and ex <= COMPOSE_BAR["gx"] and el <= COMPOSE_BAR["glam"], name


def dr_composed(dev, x, g, ps, maxit, w=W):
    torch = dev.torch
    U = dev.up(x).requires_grad_(True)
    ws = [torch.tensor(v, dtype=torch.float64, device="cuda", requires_grad=True) for v in w]
    out = gm.dr_compose(torch, dev.autograd, U, ws[0], ws[1], ps[0], ps[1], maxit)
    (dev.up(g) * out).sum().backward()
    return dev.down(U.grad), np.array([float(v.grad) for v in ws]), dev.down(out.detach())


def pd_composed(dev, x, g, loop, dims, ps, K):
    torch = dev.torch
    ws, lams = lams_of(loop, dims)
    yc = dev.up(x).requires_grad_(True)
    wt = [torch.tensor(v, dtype=torch.float64, device="cuda", requires_grad=True) for v in lams]
    out = gm.pd_compose(torch, dev.autograd, loop, yc, wt, dims, ps, K)
    (dev.up(g) * out).sum().backward()
    scale = len(dims) if loop == "pd" else 1     # (tvgen_vjp returns the gradient in ws; the composition's is in ws * scale)
    return dev.down(yc.grad), np.array([float(v.grad) for v in wt]) * scale, dev.down(out.detach())


# ---- 1. the option off: refused, nothing written --------------------------------------------------------------------------------------------
def test_off_refuses_and_writes_nothing(dev, clib):
    torch = dev.torch
    before = dev.ptv.general_p_vjp(False)
    try:
        assert dev.ptv.general_p_vjp(False) is False
        x = dev.up(draw((12, 10), 2)[0])
        with pytest.raises(NotImplementedError):
            dev.device.dr2_vjp(x, x, 0.3, p_col=1.5)
        with pytest.raises(NotImplementedError):
            dev.device.tvgen_vjp(x, x, (0.3, 0.2), (1, 2), 3, ps=(3, 1))
        g, gU, glam = dev.up(np.ones((12, 10))), torch.full_like(x, 7.0), np.full(2, 7.0)
        ns, lams, dims, norms = np.array((12, 10), dtype=np.int32), np.array([0.3, 0.2]), np.array([1.0, 2.0]), np.array([1.0, 1.5])
        torch.cuda.synchronize()
        assert clib.proxtv_DR2_TVp_vjp_dev(12, 10, x.data_ptr(), 0.3, 0.2, 1.5, 1.0, g.data_ptr(), 0, gU.data_ptr(), glam.ctypes.data, 3, 0, 0) == 0
        assert b"p = 1" in clib.proxtv_last_error() and bool((gU == 7.0).all()) and np.all(glam == 7.0)
        for which in (0, 1):
            assert clib.proxtv_PD_TVp_vjp_dev(which, x.data_ptr(), lams.ctypes.data, norms.ctypes.data, dims.ctypes.data, ns.ctypes.data, 2, 2, 3,
                                              g.data_ptr(), 0, gU.data_ptr(), glam.ctypes.data, 0, 0) == 0
            assert b"p = 1" in clib.proxtv_last_error() and bool((gU == 7.0).all()) and np.all(glam == 7.0)
    finally:
        dev.ptv.general_p_vjp(before)


# ---- 2. the option on, norms in {1, 2}: today's bits --------------------------------------------------------------------------------------
def test_on_with_norms_one_and_two_gives_the_same_bits(dev):
    torch = dev.torch
    x, g = draw((70, 130), 5)
    y3, g3 = draw((20, 30, 9), 6)
    outs = []
    before = dev.ptv.general_p_vjp(False)
    try:
        for flag in (False, True):
            dev.ptv.general_p_vjp(flag)
            got = []
            for ps in ((1, 2), (2, 2), (1, 1)):
                for tape in ("outputs", "steps"):
                    got.extend(dr_call(dev, x, g, ps, 3, tape=tape))
            got.extend(pd_call(dev, x, g, "pd2", (1, 2), (2, 1), 3))
            got.extend(pd_call(dev, y3, g3, "pd", (1, 2, 1, 3), (1, 2, 2, 1), 3))
            outs.append(got)
    finally:
        dev.ptv.general_p_vjp(before)
    assert same(outs[0], outs[1], torch)


# ---- 3. against the composition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,ps,maxit", DR_CASES)
def test_dr_against_the_composition(dev, on, shape, ps, maxit):
    x, g = dr_data(shape, ps)
    got = dr_call(dev, x, g, ps, maxit)
    assert got[1].shape == (2,)
    against(f"dr {shape} p {ps} maxit {maxit}", dev, got, dr_composed(dev, x, g, ps, maxit))


@pytest.mark.parametrize("loop,shape,dims,ps,K", PD_CASES)
def test_pd_against_the_composition(dev, on, loop, shape, dims, ps, K):
    x, g = pd_data(shape, ps)
    got = pd_call(dev, x, g, loop, dims, ps, K)
    assert got[1].shape == (len(dims),)
    against(f"{loop} {shape} dims {dims} p {ps} K {K}", dev, got, pd_composed(dev, x, g, loop, dims, ps, K))


# ---- 4. the same bits: both tapes, twice, in place, both routes ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape,ps,maxit", (((70, 130), (3, 1.5), 5), ((70, 130), (1, 1.5), 2), ((65, 3), (1.5, 2), 2), ((2, 67), (7, 1.1), 2),
                                            ((1, 40), (3, 1.5), 2), ((67, 1), (1.5, 3), 2), ((67, 1), (3, 1), 3)))
def test_dr_same_bits(dev, clib, on, shape, ps, maxit):
    torch = dev.torch
    x, g = dr_data(shape, ps)
    first = dr_call(dev, x, g, ps, maxit)
    assert same(first, dr_call(dev, x, g, ps, maxit), torch)
    assert same(first, dr_call(dev, x, g, ps, maxit, tape="steps"), torch)
    # (rows are strided: the fused route is legal there.  A column sweep runs along dimension 0, where it is legal for a single column
    # only: the (67, 1) cases are what reaches the fused DR_COL kernel)
    for route in (1, 2):
        clib.proxtv_set_option(b"tvp_vjp_route", route)
        assert same(first, dr_call(dev, x, g, ps, maxit), torch), route
        U, gg, glam = dev.up(x), dev.up(g), np.zeros(2)
        torch.cuda.synchronize()
        assert clib.proxtv_DR2_TVp_vjp_dev(shape[0], shape[1], U.data_ptr(), W[0], W[1], float(ps[0]), float(ps[1]), gg.data_ptr(), 0, gg.data_ptr(),
                                           glam.ctypes.data, maxit, 0, 0) == 1
        assert torch.equal(gg, first[0]) and np.array_equal(glam, first[1]), route


@pytest.mark.parametrize("loop,shape,dims,ps,K", (PD_CASES[0], PD_CASES[2], PD_CASES[4], PD_CASES[5], PD_CASES[6],
                                                  ("pd", (20, 30, 9), (2, 3), (1.5, 3), 1), ("pd2", (20, 30, 9), (3, 2), (3, 1.5), 2)))
def test_pd_same_bits(dev, clib, on, loop, shape, dims, ps, K):
    torch = dev.torch
    x, g = pd_data(shape, ps)
    first = pd_call(dev, x, g, loop, dims, ps, K)
    assert same(first, pd_call(dev, x, g, loop, dims, ps, K), torch)
    assert same(first, pd_call(dev, x, g, loop, dims, ps, K, tape="steps"), torch)
    P = len(dims)
    _, lams = lams_of(loop, dims)
    for route in (1, 2):
        clib.proxtv_set_option(b"tvp_vjp_route", route)
        assert same(first, pd_call(dev, x, g, loop, dims, ps, K), torch), route
        y, gg = dev.up(x), dev.up(g)
        la, dd, ns, norms, glam = np.array(lams), np.array(dims, dtype=np.float64), np.array(shape, dtype=np.int32), np.array(ps, dtype=np.float64), np.zeros(P)
        torch.cuda.synchronize()
        assert clib.proxtv_PD_TVp_vjp_dev(0 if loop == "pd2" else 1, y.data_ptr(), la.ctypes.data, norms.ctypes.data, dd.ctypes.data, ns.ctypes.data,
                                          len(shape), P, K, gg.data_ptr(), 0, gg.data_ptr(), glam.ctypes.data, 0, 0) == 1
        assert torch.equal(gg, first[0]) and np.array_equal(glam * (P if loop == "pd" else 1), first[1]), route


# ---- 5. the branch cases inside a loop ----------------------------------------------------------------------------------------------------------
def kinds(dev, operand, w, p, dim):
    """(closed, iterated): fibres of the sweep's operand that the general-p prox answers in closed form (gap exactly 0) / by iterating."""
    _, gap = dev.device.tvp_fibres(dev.up(operand), w, p, dim, return_gap=True)
    gap = dev.down(gap)
    return int(np.sum(gap == 0)), int(np.sum(gap > 0))


@pytest.mark.parametrize("case", ("constant columns", "large lambda"))
def test_branches_inside_a_loop(dev, on, case):
    """pd2 on (70, 130), first term general p along dimension 0: its first sweep's operand is the input itself."""
    shape, dims, K = (70, 130), (1, 2), 3
    x, g = draw(shape, 77)
    if case == "constant columns":
        x[:, ::3] = np.arange(0, shape[1], 3) * 0.25         # every third column exactly constant: the prox answers with the mean
        ps, ws = (1.5, 1), (0.25, 0.4)
    else:
        x *= np.array([3.0, 0.02] * (shape[1] // 2))          # every other column tiny: a penalty of 0.8 flattens those and not the others
        ps, ws = (3, 1.5), (0.8, 0.4)
    closed, iterated = kinds(dev, x, ws[0], ps[0], 0)
    print(f"{case}: {closed} fibres in closed form, {iterated} iterated")
    assert closed > 0 and iterated > 0
    torch = dev.torch
    got = dev.device.tvgen_vjp(dev.up(x), dev.up(g), ws, dims, K, "pd2", need_glam=True, need_y=True, ps=ps)
    yc = dev.up(x).requires_grad_(True)
    wt = [torch.tensor(v, dtype=torch.float64, device="cuda", requires_grad=True) for v in ws]
    out = gm.pd_compose(torch, dev.autograd, "pd2", yc, wt, dims, ps, K)
    (dev.up(g) * out).sum().backward()
    against(f"branches, {case}", dev, got, (dev.down(yc.grad), np.array([float(v.grad) for v in wt]), dev.down(out.detach())))


# ---- 6. autograd ------------------------------------------------------------------------------------------------------------------------------------
FD_SHAPE = (24, 18)


def central(loss, x, pens):
    h = gm.FD_H
    gx = np.asarray(vm.central_x(lambda v: loss(v, pens), np.ascontiguousarray(x.copy()), h)).reshape(x.shape)
    gl = []
    for i in range(len(pens)):
        up, dn = list(pens), list(pens)
        up[i] += h
        dn[i] -= h
        gl.append((loss(x, up) - loss(x, dn)) / (2 * h))
    return gx, np.array(gl)


@pytest.mark.parametrize("ps", ((1.5, 1), (3, 1.5)))
def test_autograd_tvp_2d(dev, on, ps):
    torch, maxit = dev.torch, 3
    dev.ptv.general_p(True)
    U, g = draw(FD_SHAPE, 31)
    cd = dev.up(g)
    x = dev.up(U).requires_grad_(True)
    ws = [torch.tensor(W[0], dtype=torch.float64, requires_grad=True), torch.tensor(W[1], dtype=torch.float64, device="cuda", requires_grad=True)]
    y = dev.autograd.tvp_2d(x, ws[0], ws[1], ps[0], ps[1], maxit)
    assert y.grad_fn is not None and torch.equal(y.detach(), dev.device.tvp_2d(dev.up(U), W[0], W[1], ps[0], ps[1], maxit)[0])
    assert dev.autograd.tvp_2d(dev.up(U), W[0], W[1], ps[0], ps[1], maxit).grad_fn is None
    (cd * y).sum().backward()
    gx, glam, _ = dr_call(dev, U, g, ps, maxit)
    assert torch.equal(x.grad, gx) and np.array_equal(np.array([float(w.grad) for w in ws]), glam)
    assert all(w.grad.device == w.device and w.grad.shape == () for w in ws)
    loss = lambda u, w: float((cd * dev.device.tvp_2d(dev.up(u), w[0], w[1], ps[0], ps[1], maxit)[0]).sum())   # noqa: E731
    fx, fl = central(loss, U, W)
    ex, el = float(np.max(np.abs(dev.down(x.grad) - fx))), float(np.max(np.abs(fl - glam)))
    print(f"FD tvp_2d p {ps}: |gx - fd| {ex:.2e}, |glam - fd| {el:.2e}")
    assert ex <= FD_BAR["gx"] and el <= FD_BAR["glam"]


@pytest.mark.parametrize("loop,dims,ps", (("pd2", (1, 2), (1.5, 1)), ("pd", (1, 2, 1), (3, 1.5, 1))))
def test_autograd_tvgen(dev, on, loop, dims, ps):
    torch, iters = dev.torch, 3
    dev.ptv.general_p(True)
    y0, g = draw(FD_SHAPE, 32)
    ws, _ = lams_of(loop, dims)
    assert int(dev.device.tvgen(dev.up(y0), ws, dims, iters, loop, ps=ps)[1][0]) == iters
    cd = dev.up(g)
    x = dev.up(y0).requires_grad_(True)
    wt = [torch.tensor(w, dtype=torch.float64, device="cuda", requires_grad=True) for w in ws]
    y = dev.autograd.tvgen(x, wt, dims, iters, loop, ps=ps)
    assert y.grad_fn is not None and torch.equal(y.detach(), dev.device.tvgen(dev.up(y0), ws, dims, iters, loop, ps=ps)[0])
    (cd * y).sum().backward()
    gx, glam, _ = pd_call(dev, y0, g, loop, dims, ps, iters)
    assert torch.equal(x.grad, gx) and np.array_equal(np.array([float(w.grad) for w in wt]), glam)

    def loss(u, w):
        out, info = dev.device.tvgen(dev.up(u), w, dims, iters, loop, ps=ps)
        assert int(info[0]) == iters
        return float((cd * out).sum())

    fx, fl = central(loss, y0, ws)
    ex, el = float(np.max(np.abs(dev.down(x.grad) - fx))), float(np.max(np.abs(fl - glam)))
    print(f"FD tvgen {loop} p {ps}: |gx - fd| {ex:.2e}, |glam - fd| {el:.2e}")
    assert ex <= FD_BAR["gx"] and el <= FD_BAR["glam"]


# ---- 7. refusals with the option on ---------------------------------------------------------------------------------------------------------------
def test_refusals_with_the_option_on(dev, clib, on):
    torch = dev.torch
    x = dev.up(draw((12, 10), 2)[0])
    wm = dev.up(np.full((11, 10), 0.3)), dev.up(np.full((12, 9), 0.3))
    g, gU, glam = dev.up(np.ones((12, 10))), torch.full_like(x, 7.0), np.full(2, 7.0)
    ns, lams, dims = np.array((12, 10), dtype=np.int32), np.array([0.3, 0.2]), np.array([1.0, 2.0])
    for p in (1.001, 100.0, np.inf):
        with pytest.raises(NotImplementedError, match="1.002 < p < 100"):
            dev.device.dr2_vjp(x, x, 0.3, p_row=p)
        with pytest.raises(NotImplementedError, match="1.002 < p < 100"):
            dev.device.tvgen_vjp(x, x, (0.3, 0.2), (1, 2), 3, ps=(p, 1))
        norms = np.array([1.0, p])
        torch.cuda.synchronize()
        assert clib.proxtv_DR2_TVp_vjp_dev(12, 10, x.data_ptr(), 0.3, 0.2, p, 1.0, g.data_ptr(), 0, gU.data_ptr(), glam.ctypes.data, 3, 0, 0) == 0
        assert b"1.002 < p < 100" in clib.proxtv_last_error() and bool((gU == 7.0).all()) and np.all(glam == 7.0)
        for which in (0, 1):
            assert clib.proxtv_PD_TVp_vjp_dev(which, x.data_ptr(), lams.ctypes.data, norms.ctypes.data, dims.ctypes.data, ns.ctypes.data, 2, 2, 3,
                                              g.data_ptr(), 0, gU.data_ptr(), glam.ctypes.data, 0, 0) == 0
            assert b"1.002 < p < 100" in clib.proxtv_last_error() and bool((gU == 7.0).all()) and np.all(glam == 7.0)
    for method in ("pdr", "yang"):
        with pytest.raises(NotImplementedError):
            dev.device.tvgen_vjp(x, x, (0.3, 0.2), (1, 2), 3, method=method, ps=(1.5, 1))
    with pytest.raises(ValueError):
        dev.device.dr2_vjp(x, x, 0.3, weights_col=wm[0], weights_row=wm[1], p_row=1.5)
    with pytest.raises(ValueError):
        dev.device.dr2_vjp(dev.up(np.zeros((12, 10, 2))), dev.up(np.zeros((12, 10, 2))), 0.3, p_col=3)
    # autograd wants both switches, and names the one that is missing
    xr = lambda: x.clone().requires_grad_(True)   # noqa: E731
    dev.ptv.general_p(False)
    with pytest.raises(NotImplementedError, match=r"general_p\(True\)"):
        dev.autograd.tvp_2d(xr(), 0.3, 0.3, 1.5, 1)
    with pytest.raises(NotImplementedError, match=r"general_p\(True\)"):
        dev.autograd.tvgen(xr(), (0.3, 0.2), (1, 2), ps=(1, 3))
    dev.ptv.general_p(True)
    dev.ptv.general_p_vjp(False)
    with pytest.raises(NotImplementedError, match="general_p_vjp"):
        dev.autograd.tvp_2d(xr(), 0.3, 0.3, 1.5, 1)
    with pytest.raises(NotImplementedError, match="general_p_vjp"):
        dev.autograd.tvgen(xr(), (0.3, 0.2), (1, 2), ps=(1, 3))
    dev.ptv.general_p_vjp(True)
    with pytest.raises(NotImplementedError):
        dev.autograd.tvgen(xr(), (0.3, 0.2), (1, 2), method="pdr", ps=(1, 1.5))


# ---- 8. the pool's cap ------------------------------------------------------------------------------------------------------------------------------
def test_beyond_the_pool_cap_is_refused_and_names_the_headers_bytes():
    """PROXTV_POOL_CAP_MB is read once per process: a fresh child with a 1 MiB cap."""
    env = dict(os.environ, PROXTV_POOL_CAP_MB="1", PROXTV_GENERAL_P_VJP="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "tvpg_vjp_cap_child.py")], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "CAP_CHILD_OK" in r.stdout
