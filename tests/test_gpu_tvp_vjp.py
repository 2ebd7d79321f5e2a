"""The derivatives of the Douglas-Rachford and Dykstra solves with TV-L2 terms on the GPU: proxtv_DR2_TVp_vjp_dev and
proxtv_PD_TVp_vjp_dev through device.dr2_vjp(p_col=, p_row=) / device.tvgen_vjp(ps=), and autograd.tvp_2d / autograd.tvgen(ps=).
Yardsticks: the numpy model of tests/tvp_vjp_model.py (checked against central differences in tests/test_tvp_vjp_model.py), the same
recurrences composed in torch from autograd.tv1_fibres / autograd.tv2_fibres, and central differences of the fused device solves.

The bar of the model comparisons is tvp_vjp_model.bar: the TV-L1 recurrence's 64 S L 2^-52 A (pd_vjp_model.bar) times the worst
cond(T + mu I) = (4 + mu) / (mu + 4 sin^2(pi / 2n)) over the case's TV-L2 fibres and sweeps (tests/test_tv2_vjp_host.py).

Data: tvp_vjp_model.draw_rows -- unit noise whose slices across the TV-L2 fibres alternate between two sizes, so that every case holds
fibres inside the ball (mu = 0) and active ones; every model asserts that no TV-L2 fibre lies within 1e-6 of its kink and no TV-L1 jump
where the step rule decides, so that the device and the model differentiate the same branch.

Shapes: (70, 130) (dimension-0 fibres through the transposed route, strided rows, more than one wave), (65, 3) and (2, 67) (fibres of 3
and 2 samples), (1, 40) (fibres of 1 sample; a single dimension-0 fibre), (20, 30, 9) (a middle dimension), 1 x 20000 (the long route)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import tvp_vjp_model as tp
import vjp_model as vm
from conftest import REL_TOL, rel_err

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
AMPS = (3.0, 0.02)
W = (0.3, 0.25)
DR_CASES = tuple((shape, ps, maxit) for shape in ((70, 130), (65, 3), (1, 40)) for ps in ((1, 2), (2, 1), (2, 2)) for maxit in (1, 2, 7)) + \
    tuple(((2, 67), ps, 2) for ps in ((1, 2), (2, 1), (2, 2)))
PD2_CASES = tuple(("pd2", (70, 130), tuple(range(1, len(ps) + 1)), ps, K) for ps in ((1, 2), (2, 1), (2, 2), (2,)) for K in (1, 2, 5))
PD_CASES = tuple(("pd", (20, 30, 9), dims, ps, K) for dims, ps in (((1, 2, 3), (2, 1, 1)), ((1, 2, 3), (1, 2, 2)), ((1, 2, 1, 3), (1, 1, 2, 1)))
                 for K in (1, 3))


@pytest.fixture(scope="module")
def dev(ptv):
    import torch
    from proxtv_amd import autograd, device

    class Dev:
        pass

    d = Dev()
    d.torch, d.device, d.autograd = torch, device, autograd
    d.up = lambda a: device.to_colmajor(torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda())
    d.down = lambda t: t.cpu().numpy()
    return d


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


def l2_axis(shape, dims, ps):
    """The axis whose slices draw_rows scales: one that is not a TV-L2 term's own (of more than one slice where there is one)."""
    own = {int(d) - 1 for d, p in zip(dims, ps) if p == 2}
    free = [a for a in range(len(shape)) if a not in own and shape[a] > 1]
    return free[0] if free else max(range(len(shape)), key=lambda a: shape[a])


@functools.lru_cache(maxsize=None)
def dr_model(shape, ps, maxit):
    """One Douglas-Rachford case, once: inputs, the model's forward result and gradients (shared by the tests; nobody writes into them)."""
    from oracle import cpu
    U, g = tp.draw_rows(300 + sum(shape) + 10 * ps[0] + ps[1], shape, AMPS, l2_axis(shape, (1, 2), ps))
    out, tape = tp.dr_forward(cpu.oracle(), U, W[0], W[1], ps[0], ps[1], maxit)
    tp.assert_well_defined(tape, clear=1e-6)
    gU, glam, sweeps, A = tp.dr_reverse(tape, g)
    frozen(U, g, out, gU, glam)
    return dict(x=U, g=g, out=out, gx=gU, glam=glam, tape=tape, bar=tp.bar(tape, sweeps, A), glam_bars=tp.glam_bars(tape, sweeps, A))


def lams_of(loop, dims):
    """(ws as a user passes them to tvgen, lams as the C entry point receives them)."""
    P = len(dims)
    ws = tuple((0.25 + 0.15 * i) / (P if loop == "pd" else 1) for i in range(P))
    return ws, tuple(w * (P if loop == "pd" else 1) for w in ws)


@functools.lru_cache(maxsize=None)
def pd_model(loop, shape, dims, ps, K, amps=AMPS):
    from oracle import cpu
    y, g = tp.draw_rows(500 + sum(shape) + sum(ps), shape, amps, l2_axis(shape, dims, ps))
    ws, lams = lams_of(loop, dims)
    out, tape = tp.pd_forward(cpu.oracle(), loop, y, lams, dims, ps, K)
    tp.assert_well_defined(tape, clear=1e-6)
    gy, glam, sweeps, A = tp.pd_reverse(loop, tape, g)
    frozen(y, g, out, gy, glam)
    return dict(x=y, g=g, out=out, gx=gy, glam=glam, tape=tape, ws=ws, lams=lams, bar=tp.bar(tape, sweeps, A),
                glam_bars=tp.glam_bars(tape, sweeps, A))


def worst(got, want):
    return float(np.max(np.abs(got - want))) if want.size else 0.0


def dr_call(dev, m, ps, maxit, **kw):
    gx, _, _, glam, y = dev.device.dr2_vjp(dev.up(m["x"]), dev.up(m["g"]), W[0], W[1], maxit, need_gw="sums", need_y=True, p_col=ps[0],
                                           p_row=ps[1], **kw)
    return gx, glam, y


def pd_call(dev, m, loop, dims, ps, K, **kw):
    return dev.device.tvgen_vjp(dev.up(m["x"]), dev.up(m["g"]), m["ws"], dims, K, loop, need_glam=True, need_y=True, ps=ps, **kw)


def against_model(dev, m, gx, glam, y, scale, name):
    ex, el, ey = worst(dev.down(gx), m["gx"]), np.abs(np.asarray(glam) / scale - m["glam"]), worst(dev.down(y), m["out"])
    inside, active = tp.branches(m["tape"])
    print(f"{name}: |gx - model| {ex:.2e} (bar {m['bar']:.2e}, ratio {ex / m['bar']:.4f}), |glam - model| / bar "
          f"{float(np.max(el / m['glam_bars'])):.2e}, forward {ey:.2e}, worst cond {tp.worst_cond(m['tape']):.1f}, TV-L2 fibres inside "
          f"{inside} active {active}")
    assert ex <= m["bar"], name
    assert np.all(el <= m["glam_bars"]), name
    assert rel_err(dev.down(y), m["out"]) <= REL_TOL, name     # (the parity bar against the CPU oracle)


# ---- 1. every norm 1: the bits of the TV-L1 entry points -------------------------------------------------------------------------------------
@pytest.mark.parametrize("tape", (0, 1))
def test_all_norms_one_gives_the_bits_of_the_l1_calls(dev, clib, tape):
    torch = dev.torch
    rng = np.random.default_rng(4)
    M, N = 70, 130
    U, g = dev.up(rng.standard_normal((M, N))), dev.up(rng.standard_normal((M, N)))
    outs = []
    for new in (False, True):
        s, gU, glam = torch.full_like(g, 7.0), torch.full_like(g, 7.0), np.full(2, 7.0)
        torch.cuda.synchronize()
        if new:
            rc = clib.proxtv_DR2_TVp_vjp_dev(M, N, U.data_ptr(), 0.3, 0.2, 1.0, 1.0, g.data_ptr(), s.data_ptr(), gU.data_ptr(), glam.ctypes.data, 3,
                                             tape, 0)
        else:
            rc = clib.proxtv_DR2_TV_vjp_tape_dev(M, N, 1, U.data_ptr(), 0.3, 0.2, 0, 0, g.data_ptr(), s.data_ptr(), gU.data_ptr(), 0, 0,
                                                 glam.ctypes.data, 3, tape, 0)
        assert rc == 1 and clib.proxtv_last_error() == b""
        outs.append((s, gU, glam))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])
    shape = (20, 30, 9)
    y, g = dev.up(rng.standard_normal(shape)), dev.up(rng.standard_normal(shape))
    ns = np.array(shape, dtype=np.int32)
    for which, dims in ((0, (2.0, 3.0)), (1, (1.0, 2.0, 1.0, 3.0))):
        P = len(dims)
        lams, dd, ones = np.array([0.3, 0.2, 0.25, 0.4][:P]), np.array(dims), np.ones(P)
        outs = []
        for norms in (None, ones, "old"):
            x, gy, glam = torch.full_like(g, 7.0), torch.full_like(g, 7.0), np.full(P, 7.0)
            torch.cuda.synchronize()
            if isinstance(norms, str):
                rc = clib.proxtv_PD_TV_vjp_tape_dev(which, y.data_ptr(), lams.ctypes.data, dd.ctypes.data, ns.ctypes.data, 3, P, 3, g.data_ptr(),
                                                    x.data_ptr(), gy.data_ptr(), glam.ctypes.data, tape, 0)
            else:
                rc = clib.proxtv_PD_TVp_vjp_dev(which, y.data_ptr(), lams.ctypes.data, 0 if norms is None else norms.ctypes.data, dd.ctypes.data,
                                                ns.ctypes.data, 3, P, 3, g.data_ptr(), x.data_ptr(), gy.data_ptr(), glam.ctypes.data, tape, 0)
            assert rc == 1 and clib.proxtv_last_error() == b""
            outs.append((x, gy, glam))
        for o in outs[:2]:
            assert torch.equal(o[0], outs[2][0]) and torch.equal(o[1], outs[2][1]) and np.array_equal(o[2], outs[2][2])


# ---- 2. against the numpy model ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,ps,maxit", DR_CASES)
def test_dr_against_the_model(dev, shape, ps, maxit):
    m = dr_model(shape, ps, maxit)
    gx, glam, y = dr_call(dev, m, ps, maxit)
    assert glam.shape == (2,)
    against_model(dev, m, gx, glam, y, 1, f"dr {shape} p {ps} maxit {maxit}")


@pytest.mark.parametrize("loop,shape,dims,ps,K", PD2_CASES + PD_CASES)
def test_pd_against_the_model(dev, loop, shape, dims, ps, K):
    m = pd_model(loop, shape, dims, ps, K)
    gx, glam, y = pd_call(dev, m, loop, dims, ps, K)
    assert glam.shape == (len(dims),)
    against_model(dev, m, gx, glam, y, len(dims) if loop == "pd" else 1, f"{loop} {shape} dims {dims} p {ps} K {K}")


def test_fibre_lengths_and_routes_occur():
    """What the cases above are chosen for: TV-L2 fibres of 1, 2 and 3 samples, along dimension 0, a middle and the last dimension."""
    lengths, dims = set(), set()
    for shape, ps, _ in DR_CASES:
        for d, p in enumerate(ps):
            if p == 2:
                lengths.add(shape[d])
                dims.add((d, len(shape)))
    for _, shape, ds, ps, _ in PD2_CASES + PD_CASES:
        for d, p in zip(ds, ps):
            if p == 2:
                dims.add((d - 1, len(shape)))
    assert {1, 2, 3} <= lengths and {(0, 2), (1, 2), (0, 3), (1, 3), (2, 3)} <= dims


# ---- 3. against the composition on the device --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", ((1, 2), (2, 2)))
def test_dr_against_the_torch_composition(dev, ps):
    torch = dev.torch
    shape, maxit = (70, 130), 2
    m = dr_model(shape, ps, maxit)
    gx, glam, y = dr_call(dev, m, ps, maxit)
    U = dev.up(m["x"]).requires_grad_(True)
    ws = [torch.tensor(w, dtype=torch.float64, device="cuda", requires_grad=True) for w in W]
    out = tp.dr_compose(torch, dev.autograd, U, ws[0], ws[1], ps[0], ps[1], maxit)
    (dev.up(m["g"]) * out).sum().backward()
    ex, ey = worst(dev.down(gx), dev.down(U.grad)), worst(dev.down(y), dev.down(out.detach()))
    el = np.abs(glam - np.array([float(w.grad) for w in ws]))
    print(f"dr {shape} p {ps}: |gx - composition| {ex:.2e} (bar {m['bar']:.2e}), penalties / bar {float(np.max(el / m['glam_bars'])):.2e}, forward {ey:.2e}")
    assert ex <= m["bar"] and np.all(el <= m["glam_bars"]) and ey <= m["bar"]


@pytest.mark.parametrize("loop,shape,dims,ps,K", (PD2_CASES[7], PD_CASES[3], PD_CASES[5]))
def test_pd_against_the_torch_composition(dev, loop, shape, dims, ps, K):
    torch = dev.torch
    m = pd_model(loop, shape, dims, ps, K)
    gx, glam, y = pd_call(dev, m, loop, dims, ps, K)
    yc = dev.up(m["x"]).requires_grad_(True)
    ws = [torch.tensor(w, dtype=torch.float64, device="cuda", requires_grad=True) for w in m["lams"]]
    out = tp.pd_compose(torch, dev.autograd, loop, yc, ws, dims, ps, K)
    (dev.up(m["g"]) * out).sum().backward()
    scale = len(dims) if loop == "pd" else 1
    ex, ey = worst(dev.down(gx), dev.down(yc.grad)), worst(dev.down(y), dev.down(out.detach()))
    el = np.abs(glam / scale - np.array([float(w.grad) for w in ws]))
    print(f"{loop} {shape} p {ps} K {K}: |gx - composition| {ex:.2e} (bar {m['bar']:.2e}), penalties / bar {float(np.max(el / m['glam_bars'])):.2e}, "
          f"forward {ey:.2e}")
    assert ex <= m["bar"] and np.all(el <= m["glam_bars"]) and ey <= m["bar"]


# ---- 4. autograd ---------------------------------------------------------------------------------------------------------------------------------
FD_SHAPE = (24, 18)


def central(loss, x, pens, dev):
    """Central differences (h = 1e-5) of loss(x, pens) in every entry of x and every penalty."""
    h = tp.FD_H
    gx = vm.central_x(lambda v: loss(v, pens), np.ascontiguousarray(x.copy()), h)
    gl = []
    for i in range(len(pens)):
        up, dn = list(pens), list(pens)
        up[i] += h
        dn[i] -= h
        gl.append((loss(x, up) - loss(x, dn)) / (2 * h))
    return gx, np.array(gl)


@pytest.mark.parametrize("ps", ((1, 2), (2, 2)))
def test_autograd_tvp_2d(dev, ps):
    """Forward: the bits of device.tvp_2d.  Gradients in x and both penalties against central differences of device.tvp_2d, bar 1e-7; the
    inputs keep every TV-L2 fibre 20 % away from its kink in every sweep (the model says so)."""
    from oracle import cpu
    torch, maxit = dev.torch, 3
    U, g = tp.draw_rows(3, FD_SHAPE, AMPS, l2_axis(FD_SHAPE, (1, 2), ps))
    tp.assert_well_defined(tp.dr_forward(cpu.oracle(), U, W[0], W[1], ps[0], ps[1], maxit)[1], hi=1e-4)
    cd = dev.up(g)
    x = dev.up(U).requires_grad_(True)
    ws = [torch.tensor(W[0], dtype=torch.float64, requires_grad=True), torch.tensor(W[1], dtype=torch.float64, device="cuda", requires_grad=True)]
    y = dev.autograd.tvp_2d(x, ws[0], ws[1], ps[0], ps[1], maxit)
    y0 = dev.device.tvp_2d(dev.up(U), W[0], W[1], ps[0], ps[1], maxit)[0]
    assert y.grad_fn is not None and torch.equal(y.detach(), y0)
    assert dev.autograd.tvp_2d(dev.up(U), W[0], W[1], ps[0], ps[1], maxit).grad_fn is None
    (cd * y).sum().backward()
    assert all(w.grad.device == w.device and w.grad.shape == () for w in ws) and dev.device._is_colmajor(x.grad)
    loss = lambda u, w: float((cd * dev.device.tvp_2d(dev.up(u), w[0], w[1], ps[0], ps[1], maxit)[0]).sum())   # noqa: E731
    fx, fl = central(loss, U, W, dev)
    ex, el = worst(dev.down(x.grad), fx), float(np.max(np.abs(fl - np.array([float(w.grad) for w in ws]))))
    print(f"tvp_2d p {ps}: |gx - fd| {ex:.2e}, |glam - fd| {el:.2e} (bar {tp.FD_TOL:.0e})")
    assert ex <= tp.FD_TOL and el <= tp.FD_TOL
    # the steps tape: the same bits
    x2 = dev.up(U).requires_grad_(True)
    (cd * dev.autograd.tvp_2d(x2, W[0], W[1], ps[0], ps[1], maxit, tape="steps")).sum().backward()
    assert torch.equal(x2.grad, x.grad)


@pytest.mark.parametrize("seed,loop,dims,ps", ((36, "pd2", (1, 2), (2, 1)), (4, "pd", (1, 2, 1), (1, 2, 2))))
def test_autograd_tvgen_with_norms(dev, seed, loop, dims, ps):
    """As above for device.tvgen(ps=...); the seeds are chosen on the CPU so that the 20 % clearance holds."""
    from oracle import cpu
    torch, iters = dev.torch, 3
    y0, g = tp.draw_rows(seed, FD_SHAPE, AMPS, l2_axis(FD_SHAPE, dims, ps))
    ws, lams = lams_of(loop, dims)
    K = int(dev.device.tvgen(dev.up(y0), ws, dims, iters, loop, ps=ps)[1][0])
    assert K == iters
    tp.assert_well_defined(tp.pd_forward(cpu.oracle(), loop, y0, lams, dims, ps, K)[1], hi=1e-4)
    cd = dev.up(g)
    x = dev.up(y0).requires_grad_(True)
    wt = [torch.tensor(w, dtype=torch.float64, device="cuda", requires_grad=True) for w in ws]
    y = dev.autograd.tvgen(x, wt, dims, iters, loop, ps=ps)
    assert y.grad_fn is not None and torch.equal(y.detach(), dev.device.tvgen(dev.up(y0), ws, dims, iters, loop, ps=ps)[0])
    (cd * y).sum().backward()

    def loss(u, w):
        out, info = dev.device.tvgen(dev.up(u), w, dims, iters, loop, ps=ps)
        assert int(info[0]) == K
        return float((cd * out).sum())

    fx, fl = central(loss, y0, ws, dev)
    ex, el = worst(dev.down(x.grad), fx), float(np.max(np.abs(fl - np.array([float(w.grad) for w in wt]))))
    print(f"tvgen {loop} dims {dims} p {ps}: |gx - fd| {ex:.2e}, |glam - fd| {el:.2e} (bar {tp.FD_TOL:.0e})")
    assert ex <= tp.FD_TOL and el <= tp.FD_TOL


# ---- 5. / 6. the two tapes, twice, in place -----------------------------------------------------------------------------------------------------
def same(a, b, torch):
    return all(torch.equal(u, v) if isinstance(u, torch.Tensor) else np.array_equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("shape,ps,maxit", (((70, 130), (1, 2), 7), ((70, 130), (2, 1), 2), ((65, 3), (2, 2), 2), ((1, 40), (2, 2), 1)))
def test_dr_same_bits_both_tapes_twice_and_in_place(dev, clib, shape, ps, maxit):
    torch = dev.torch
    m = dr_model(shape, ps, maxit)
    first = dr_call(dev, m, ps, maxit)
    assert same(first, dr_call(dev, m, ps, maxit), torch)
    assert same(first, dr_call(dev, m, ps, maxit, tape="steps"), torch)
    U, g, glam = dev.up(m["x"]), dev.up(m["g"]), np.zeros(2)
    torch.cuda.synchronize()
    assert clib.proxtv_DR2_TVp_vjp_dev(shape[0], shape[1], U.data_ptr(), W[0], W[1], float(ps[0]), float(ps[1]), g.data_ptr(), 0, g.data_ptr(),
                                       glam.ctypes.data, maxit, 0, 0) == 1
    assert torch.equal(g, first[0]) and np.array_equal(glam, first[1])


@pytest.mark.parametrize("loop,shape,dims,ps,K", (PD2_CASES[2], PD2_CASES[8], PD2_CASES[9], PD_CASES[0], PD_CASES[1], PD_CASES[5]))
def test_pd_same_bits_both_tapes_twice_and_in_place(dev, clib, loop, shape, dims, ps, K):
    torch = dev.torch
    m = pd_model(loop, shape, dims, ps, K)
    first = pd_call(dev, m, loop, dims, ps, K)
    assert same(first, pd_call(dev, m, loop, dims, ps, K), torch)
    assert same(first, pd_call(dev, m, loop, dims, ps, K, tape="steps"), torch)
    y, g, P = dev.up(m["x"]), dev.up(m["g"]), len(dims)
    lams, dd, ns, norms, glam = np.array(m["lams"]), np.array(dims, dtype=np.float64), np.array(shape, dtype=np.int32), np.array(ps, dtype=np.float64), np.zeros(P)
    torch.cuda.synchronize()
    assert clib.proxtv_PD_TVp_vjp_dev(0 if loop == "pd2" else 1, y.data_ptr(), lams.ctypes.data, norms.ctypes.data, dd.ctypes.data, ns.ctypes.data,
                                      len(shape), P, K, g.data_ptr(), 0, g.data_ptr(), glam.ctypes.data, 0, 0) == 1
    assert torch.equal(g, first[0]) and np.array_equal(glam * (P if loop == "pd" else 1), first[1])


# ---- 7. the long route ---------------------------------------------------------------------------------------------------------------------------
def test_long_fibre(dev):
    """One contiguous fibre of 20000 samples (tv2.hip solves it parallel inside the fibre): the plain kernel and a pointwise write-out."""
    loop, shape, dims, ps, K = "pd2", (1, 20000), (2,), (2,), 1
    m = pd_model(loop, shape, dims, ps, K, amps=(1.0,))
    assert tp.branches(m["tape"]) == (0, 1)
    gx, glam, y = pd_call(dev, m, loop, dims, ps, K)
    against_model(dev, m, gx, glam, y, 1, "pd2 1 x 20000")


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev, clib):
    torch = dev.torch
    x = dev.up(np.random.default_rng(2).standard_normal((12, 10)))
    wm = dev.up(np.full((11, 10), 0.3)), dev.up(np.full((12, 9), 0.3))
    with pytest.raises(NotImplementedError):
        dev.device.tvp_2d(x, 0.3, 0.3, 1.5, 1)
    with pytest.raises(NotImplementedError):
        dev.device.dr2_vjp(x, x, 0.3, p_col=1, p_row=1.5)
    with pytest.raises(NotImplementedError):
        dev.device.tvgen(x, (0.3, 0.2), (1, 2), ps=(1, 1.5))
    with pytest.raises(NotImplementedError):
        dev.device.tvgen_vjp(x, x, (0.3, 0.2), (1, 2), 3, ps=(1.5, 2))
    with pytest.raises(NotImplementedError):
        dev.autograd.tvp_2d(x.clone().requires_grad_(True), 0.3, 0.3, 3, 2)
    with pytest.raises(NotImplementedError):
        dev.autograd.tvgen(x.clone().requires_grad_(True), (0.3, 0.2), (1, 2), ps=(2, 1.5))
    with pytest.raises(ValueError):
        dev.device.dr2_vjp(x, x, 0.3, weights_col=wm[0], weights_row=wm[1], p_row=2)
    with pytest.raises(NotImplementedError):
        dev.autograd.tvgen(x.clone().requires_grad_(True), (0.3, 0.2), (1, 2), method="pdr", ps=(1, 2))
    with pytest.raises(NotImplementedError):
        dev.device.tvgen_vjp(x, x, (0.3, 0.2), (1, 2), 3, method="yang", ps=(1, 2))
    # the C entries: a norm outside {1, 2} returns 0 and writes nothing
    g, gU, glam = dev.up(np.ones((12, 10))), torch.full_like(x, 7.0), np.full(2, 7.0)
    ns, lams, dims, norms = np.array((12, 10), dtype=np.int32), np.array([0.3, 0.2]), np.array([1.0, 2.0]), np.array([2.0, 1.5])
    torch.cuda.synchronize()
    assert clib.proxtv_DR2_TVp_vjp_dev(12, 10, x.data_ptr(), 0.3, 0.2, 2.0, 3.0, g.data_ptr(), 0, gU.data_ptr(), glam.ctypes.data, 3, 0, 0) == 0
    assert b"p = 1" in clib.proxtv_last_error() and bool((gU == 7.0).all()) and np.all(glam == 7.0)
    assert clib.proxtv_PD_TVp_vjp_dev(0, x.data_ptr(), lams.ctypes.data, norms.ctypes.data, dims.ctypes.data, ns.ctypes.data, 2, 2, 3, g.data_ptr(), 0,
                                      gU.data_ptr(), glam.ctypes.data, 0, 0) == 0
    assert b"p = 1" in clib.proxtv_last_error() and bool((gU == 7.0).all()) and np.all(glam == 7.0)
    # an empty array returns 1
    e = np.array((0, 4), dtype=np.int32)
    assert clib.proxtv_DR2_TVp_vjp_dev(0, 4, 0, 0.3, 0.2, 2.0, 1.0, 0, 0, gU.data_ptr(), glam.ctypes.data, 3, 0, 0) == 1
    norms[1] = 1.0
    assert clib.proxtv_PD_TVp_vjp_dev(1, 0, lams.ctypes.data, norms.ctypes.data, dims.ctypes.data, e.ctypes.data, 2, 2, 3, 0, 0, gU.data_ptr(),
                                      glam.ctypes.data, 0, 0) == 1
    assert clib.proxtv_last_error() == b"" and bool((gU == 7.0).all()) and np.all(glam == 7.0)


def test_a_tape_beyond_the_pool_cap_is_refused_and_names_the_headers_bytes():
    """PROXTV_POOL_CAP_MB is read once per process: a fresh child with a 1 MiB cap.  The bytes the refusals name are the header's formula,
    under both tapes."""
    env = dict(os.environ, PROXTV_POOL_CAP_MB="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "tvp_vjp_cap_child.py")], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "CAP_CHILD_OK" in r.stdout
