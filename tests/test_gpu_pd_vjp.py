"""The derivative of the two Dykstra loops behind tvgen on the GPU: proxtv_PD_TV_vjp_dev through device.tvgen_vjp, and autograd.tvgen.
Yardsticks: the numpy model of tests/pd_vjp_model.py (checked against central differences in tests/test_pd_vjp_model.py), central
differences of the fused device solves themselves, and the recurrences composed in torch from autograd.tv1_fibres.

The bar of the model comparisons is pd_vjp_model.bar: 64 S L 2^-52 A per element of gy -- the certifier's rounding rule per sum, once per
reverse sweep (S sweeps, L the longest fibre), A the largest 2-norm of any cotangent of the MODEL's reverse pass.  A penalty's gradient is
a sum, over its K sweeps and its E edges, of differences of two means, each within the bar: 2 K E times the bar.

Shapes: a contiguous fibre longer than one LDS stage of 64 chunks (1040, 5); strided fibres on both sides of 64 to a wave (17, 63, 3) and
(17, 65, 3); fibre lengths 1, 2, 15, 16, 17 in (16, 1, 7) and (2, 17, 15); a plain (70, 130)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import pd_vjp_model as pm
import vjp_model as vm
from conftest import REL_TOL, rel_err

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ((1040, 5), (17, 63, 3), (17, 65, 3), (16, 1, 7), (2, 17, 15), (70, 130))
LOOP_TERMS = (("pd2", 1), ("pd2", 2), ("pd", 1), ("pd", 2), ("pd", 3), ("pd", 4))
ITERS = (1, 2, 7)
MODEL_CASES = tuple((shape, loop, P, K) for shape in SHAPES for loop, P in LOOP_TERMS for K in ITERS)


def terms(shape, loop, P):
    """(ws, ds) of a case, as a user passes them to tvgen: term i along dimension (i + start) mod nds, so that a fourth term shares a
    dimension with the first; the two-term loop starts one dimension up, so that both loops sweep every dimension of the 3-D shapes."""
    start = 1 if loop == "pd2" else 0
    ds = tuple((i + start) % len(shape) + 1 for i in range(P))
    ws = tuple((0.25 + 0.15 * i) / (P if loop == "pd" else 1) for i in range(P))
    return ws, ds


def passed(loop, ws):
    """The penalties as the C entry point receives them."""
    return tuple(w * len(ws) for w in ws) if loop == "pd" else tuple(ws)


@pytest.fixture(scope="module")
def dev(ptv):
    import torch
    from proxtv_amd import device

    class Dev:
        pass

    d = Dev()
    d.torch, d.device = torch, device
    d.up = lambda a: device.to_colmajor(torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda())
    d.down = lambda t: t.cpu().numpy()
    return d


@functools.lru_cache(maxsize=None)
def data(shape):
    y, g = pm.draw(100 + len(shape) + sum(shape), shape)
    y.setflags(write=False)
    g.setflags(write=False)
    return y, g


@functools.lru_cache(maxsize=None)
def model(shape, loop, P, K):
    """One case, once: inputs, the model's forward result and gradients (shared by the tests; nobody writes into them)."""
    from oracle import cpu
    y, g = data(shape)
    ws, ds = terms(shape, loop, P)
    lams = passed(loop, ws)
    out, tape = pm.forward(cpu.oracle(), loop, y, lams, ds, K)
    pm.assert_tape_unambiguous(tape, ds)
    gy, glam, sweeps, A = pm.reverse(loop, tape, g, ds)
    for a in (out, gy, glam):
        a.setflags(write=False)
    edges = [y.size // shape[d - 1] * (shape[d - 1] - 1) for d in ds]
    return dict(y=y, g=g, ws=ws, ds=ds, lams=lams, out=out, gy=gy, glam=glam, K=K, loop=loop, edges=edges, sweeps=sweeps, A=A,
                bar=pm.bar(shape, ds, sweeps, A))


def call(dev, m, **kw):
    kw.setdefault("need_glam", True)
    kw.setdefault("need_y", True)
    return dev.device.tvgen_vjp(dev.up(m["y"]), dev.up(m["g"]), m["ws"], m["ds"], m["K"], m["loop"], **kw)


def worst(got, want):
    return float(np.max(np.abs(got - want))) if want.size else 0.0


def glam_bars(m):
    """Per penalty, in the penalties as the C entry point receives them: 2 K E bars (module docstring); at least one bar."""
    return np.array([2.0 * m["K"] * max(e, 1) * m["bar"] for e in m["edges"]])


# ---- 1. against the numpy model --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,loop,P,K", MODEL_CASES)
def test_against_the_model(dev, shape, loop, P, K):
    m = model(shape, loop, P, K)
    gx, glam, y = call(dev, m)
    scale = len(m["ws"]) if loop == "pd" else 1          # (device.tvgen_vjp answers in the user's penalties)
    ex = worst(dev.down(gx), m["gy"])
    el = np.abs(glam / scale - m["glam"])
    ey = worst(dev.down(y), m["out"])
    print(f"{shape} {loop} P {P} K {K}: |gy - model| {ex:.2e} (bar {m['bar']:.2e}, ratio {ex / m['bar']:.3f}), |glam - model| / bar "
          f"{float(np.max(el / glam_bars(m))):.2e}, forward {ey:.2e}, A / |g| {m['A'] / np.linalg.norm(m['g']):.2f}")
    assert glam.shape == (P,)
    assert ex <= m["bar"]
    assert np.all(el <= glam_bars(m))
    assert rel_err(dev.down(y), m["out"]) <= REL_TOL     # (the parity bar against the CPU oracle; against device.tvgen: test_forward_result)


# ---- 2. against central differences of the fused solves -------------------------------------------------------------------------------
FD_SAMPLES = 96


def fused_loss(dev, y, g, ws, ds, loop):
    """(K, cotangent on the device, loss): the fused solve with max_iters = 7, the count it reports, and sum(g * solve) as a function of
    the data and the penalties.  A perturbed solve that reported another count would be a step of the stopping rule: a precondition."""
    cd = dev.up(g)
    K = int(dev.device.tvgen(dev.up(y), ws, ds, 7, loop)[1][0])
    assert 1 <= K <= 7

    def loss(u, w=ws):
        out, inf = dev.device.tvgen(dev.up(u), w, ds, 7, loop)
        assert int(inf[0]) == K
        return float((cd * out).sum())

    return K, cd, loss


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("loop,P", (("pd2", 2), ("pd", 3)))
def test_gy_against_central_differences_of_the_device_solves(dev, shape, loop, P):
    """Unit noise, the data of the model comparisons.  Every entry of y on the shapes of up to 600 entries; on the larger ones a fixed
    sample of 96 entries (two fused solves per entry): the perturbation of one entry moves its neighbourhood alone.  An entry whose
    quotient misses the bar is put to the model: only where its perturbation changes a step of a taped sweep output -- a kink within h,
    where the solve has no derivative -- is it set aside, and at most one entry in a hundred may be."""
    from oracle import cpu
    y, g = data(shape)
    ws, ds = terms(shape, loop, P)
    h = vm.FD_H
    K, cd, loss = fused_loss(dev, y, g, ws, ds, loop)
    tape = pm.forward(cpu.oracle(), loop, y, passed(loop, ws), ds, K)[1]
    pm.assert_tape_unambiguous(tape, ds)
    base, kinks = pm.step_patterns(tape, ds), []
    gx = dev.down(dev.device.tvgen_vjp(dev.up(y), cd, ws, ds, K, loop)[0])
    flat = np.arange(y.size) if y.size <= 600 else np.random.default_rng(5).choice(y.size, FD_SAMPLES, replace=False)
    u = y.copy()
    ex = 0.0
    for i in flat:
        idx = np.unravel_index(i, shape)
        keep = u[idx]
        u[idx] = keep + h
        up = loss(u)
        u[idx] = keep - h
        dn = loss(u)
        u[idx] = keep
        e = abs((up - dn) / (2 * h) - gx[idx])
        if e > vm.FD_TOL:
            # a kink within h of the data?  Asked of the model, which knows nothing of the device's derivative: does the perturbation of
            # this entry change a step of any taped sweep output?  There the solve is not differentiable and the quotient says nothing.
            moved = False
            for v in (keep + h, keep - h):
                u[idx] = v
                moved = moved or not pm.same_patterns(base, pm.step_patterns(pm.forward(cpu.oracle(), loop, u, passed(loop, ws), ds, K)[1], ds))
            u[idx] = keep
            assert moved, (idx, e)
            kinks.append((idx, e))
            continue
        ex = max(ex, e)
    print(f"{shape} {loop} P {P} K {K}: |gy - fd| {ex:.2e} over {len(flat)} entries (bar {vm.FD_TOL:.0e}); at a kink: {kinks}")
    assert ex <= vm.FD_TOL and len(kinks) <= max(1, len(flat) // 100)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("loop,P", (("pd2", 2), ("pd", 3)))
def test_glam_against_central_differences_of_the_device_solves(dev, shape, loop, P):
    """Every penalty.  A penalty moves every segment of every sweep at once: on unit noise of these sizes some jump always lies within h
    of vanishing and the difference quotient straddles a kink, where it says nothing (6 of the 12 cases here, by the model).  So the data
    are pd_vjp_model.draw_blocks' (constant on blocks of 5).  Preconditions, checked through the model: every jump of every taped sweep
    output is nothing or at least 1e-4 (ten h), and no penalty's perturbation changes a step of any.  (Such data suit the penalties
    only: inside a block of a monotone staircase the dual sits AT the penalty, and the perturbation of one entry is itself a kink.)"""
    from oracle import cpu
    y, g = pm.draw_blocks(7, shape)
    ws, ds = terms(shape, loop, P)
    h = vm.FD_H
    K, cd, loss = fused_loss(dev, y, g, ws, ds, loop)
    glam = dev.device.tvgen_vjp(dev.up(y), cd, ws, ds, K, loop, need_glam=True)[1]
    tape = pm.forward(cpu.oracle(), loop, y, passed(loop, ws), ds, K)[1]
    pm.assert_tape_unambiguous(tape, ds, hi=1e-4)
    base = pm.step_patterns(tape, ds)
    assert sum(int(p.sum()) for p in base) > 0
    el = 0.0
    for i in range(P):
        wu, wd = list(ws), list(ws)
        wu[i] += h
        wd[i] -= h
        for w in (wu, wd):
            assert pm.same_patterns(base, pm.step_patterns(pm.forward(cpu.oracle(), loop, y, passed(loop, tuple(w)), ds, K)[1], ds)), (i, w)
        el = max(el, abs((loss(y, wu) - loss(y, wd)) / (2 * h) - glam[i]))
    print(f"{shape} {loop} P {P} K {K}: |glam - fd| {el:.2e} (bar {vm.FD_TOL:.0e})")
    assert el <= vm.FD_TOL


# ---- 3. autograd against the recurrence composed in torch ------------------------------------------------------------------------------
def test_autograd_against_the_torch_composition(dev):
    from proxtv_amd import autograd
    torch = dev.torch
    shape, loop, P = (20, 26, 14), "pd", 3
    ws, ds = terms(shape, loop, P)
    x = dev.up(data(shape)[0])
    y0, info = dev.device.tvgen(x, ws, ds, 6)
    K = int(info[0])
    m = model(shape, loop, P, K)
    assert K == 6 and autograd.tvgen(x, ws, ds, 6).grad_fn is None
    with torch.no_grad():
        assert autograd.tvgen(x.clone().requires_grad_(True), ws, ds, 6).grad_fn is None
    # native: one penalty on the CPU (its gradient comes back there), one on the GPU, one through a tensor used nowhere else
    xt = x.clone().requires_grad_(True)
    wt = [torch.tensor(ws[0], dtype=torch.float64, requires_grad=True), torch.tensor(ws[1], dtype=torch.float64, device="cuda", requires_grad=True),
          torch.tensor(ws[2], dtype=torch.float64, device="cuda", requires_grad=True)]
    y = autograd.tvgen(xt, wt, ds, 6)
    assert y.grad_fn is not None and torch.equal(y.detach(), y0)
    (dev.up(m["g"]) * y).sum().backward()
    assert xt.grad.dtype == torch.float64 and xt.grad.device == xt.device and dev.device._is_colmajor(xt.grad)
    assert all(w.grad.device == w.device and w.grad.shape == () and w.grad.dtype == torch.float64 for w in wt)
    # composed: the loop in torch on the penalties the library works with (ws * P), each a function of the user's
    xc = x.clone().requires_grad_(True)
    wc = [torch.tensor(w, dtype=torch.float64, device="cuda", requires_grad=True) for w in ws]
    out = pm.compose(torch, autograd, loop, xc, [w * P for w in wc], ds, K)
    (dev.up(m["g"]) * out).sum().backward()
    ex = worst(dev.down(xt.grad), dev.down(xc.grad))
    el = np.array([abs(float(a.grad) - float(b.grad)) for a, b in zip(wt, wc)]) / P
    print(f"|gx - composition| {ex:.2e} (bar {m['bar']:.2e}), penalties / bar {float(np.max(el / glam_bars(m))):.2e}, "
          f"forward {worst(dev.down(y0), dev.down(out.detach())):.2e}")
    assert ex <= m["bar"] and np.all(el <= glam_bars(m))
    assert worst(dev.down(xt.grad), m["gy"]) <= m["bar"]
    assert np.all(np.abs(np.array([float(w.grad) for w in wt]) / P - m["glam"]) <= glam_bars(m))


def test_autograd_two_terms_one_tensor_and_refusals(dev):
    from proxtv_amd import autograd
    torch = dev.torch
    shape = (70, 130)
    ws, ds = terms(shape, "pd2", 2)
    x = dev.up(data(shape)[0])
    _, info = dev.device.tvgen(x, ws, ds, 7)
    m = model(shape, "pd2", 2, int(info[0]))
    w0 = torch.tensor(ws[0], dtype=torch.float64, device="cuda", requires_grad=True)
    y = autograd.tvgen(x, [w0, ws[1]], ds, 7)            # only a penalty asks
    (dev.up(m["g"]) * y).sum().backward()
    assert abs(float(w0.grad) - m["glam"][0]) <= glam_bars(m)[0]
    with pytest.raises(NotImplementedError):
        autograd.tvgen(x.clone().requires_grad_(True), ws, ds, 7, method="pdr")
    with pytest.raises(NotImplementedError):
        dev.device.tvgen_vjp(x, x, ws, ds, 3, method="yang")
    with pytest.raises(ValueError):
        autograd.tvgen(x, [torch.tensor([0.3], dtype=torch.float64), 0.2], ds)
    with pytest.raises(ValueError):
        dev.device.tvgen_vjp(x, dev.up(np.ones((70, 131))), ws, ds, 3)


# ---- 4. reproducibility ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,loop,P,K", (((70, 130), "pd2", 2, 7), ((70, 130), "pd2", 1, 1), ((17, 65, 3), "pd", 3, 1), ((17, 65, 3), "pd", 4, 2),
                                            ((1040, 5), "pd", 2, 7)))
def test_same_bits_every_call_and_in_place(dev, clib, shape, loop, P, K):
    torch = dev.torch
    m = model(shape, loop, P, K)
    first, again = call(dev, m), call(dev, m)
    for a, b in zip(first, again):
        assert torch.equal(a, b) if isinstance(a, torch.Tensor) else np.array_equal(a, b)
    # gy is g: the C-ABI directly (device.tvgen_vjp always returns a fresh gx)
    y, g = dev.up(m["y"]), dev.up(m["g"])
    lams, dims, ns = np.array(m["lams"]), np.array(m["ds"], dtype=np.float64), np.array(shape, dtype=np.int32)
    glam = np.zeros(P)
    torch.cuda.synchronize()
    assert clib.proxtv_PD_TV_vjp_dev(0 if loop == "pd2" else 1, y.data_ptr(), lams.ctypes.data, dims.ctypes.data, ns.ctypes.data, len(shape), P, K,
                                     g.data_ptr(), 0, g.data_ptr(), glam.ctypes.data, 0) == 1
    assert torch.equal(g, first[0]) and np.array_equal(glam * (P if loop == "pd" else 1), first[1])


# ---- 5. the forward result ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("loop,P", LOOP_TERMS)
def test_forward_result(dev, shape, loop, P):
    y = dev.up(data(shape)[0])
    ws, ds = terms(shape, loop, P)
    fused, info = dev.device.tvgen(y, ws, ds, 7, loop)
    _, _, own = dev.device.tvgen_vjp(y, dev.up(data(shape)[1]), ws, ds, int(info[0]), loop, need_y=True)
    e = worst(dev.down(own), dev.down(fused))
    print(f"{shape} {loop} P {P} K {int(info[0])}: |x - device.tvgen| {e:.2e}")
    assert e <= 1e-12 * float(y.abs().max())


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(dev, clib):
    torch = dev.torch
    shape = (6, 4, 3)
    n = 72
    y, g = dev.up(np.arange(72.0).reshape(shape)), dev.up(np.ones(shape))
    x, gy = torch.full_like(g, 7.0), torch.full_like(g, 7.0)
    glam = np.full(3, 7.0)
    ns = np.array(shape, dtype=np.int32)
    torch.cuda.synchronize()     # (the C calls below run on the library's own stream)

    def go(which=1, yy=y, cot=g, out=x, gout=gy, dims=(1.0, 2.0, 3.0), npen=3, iters=2):
        p = lambda t: 0 if t is None else t.data_ptr()   # noqa: E731
        lams, dd = np.array([0.3, 0.2, 0.4]), np.array(dims)
        return clib.proxtv_PD_TV_vjp_dev(which, p(yy), lams.ctypes.data, dd.ctypes.data, ns.ctypes.data, 3, npen, iters, p(cot), p(out), p(gout),
                                         glam.ctypes.data, 0)

    def refused(why, **kw):
        assert go(**kw) == 0 and why in clib.proxtv_last_error(), (why, kw, clib.proxtv_last_error())
        for t in (x, gy):
            assert bool((t == 7.0).all()), why
        assert np.all(glam == 7.0), why
        assert bool((y == dev.up(np.arange(72.0).reshape(shape))).all()) and bool((g == 1.0).all())

    refused(b"iters", iters=0)
    refused(b"iters", iters=-4)
    refused(b"1 or 2 penalties", which=0)
    refused(b"which", which=2)
    refused(b"at least one", npen=0)
    refused(b"out of range", dims=(1.0, 4.0, 3.0))
    refused(b"out of range", dims=(0.0, 2.0, 3.0))
    refused(b"required", yy=None)
    refused(b"required", cot=None)
    refused(b"required", gout=None)
    refused(b"overlaps", out=y)
    refused(b"overlaps", gout=y)
    refused(b"overlaps", out=g)
    refused(b"overlaps", out=gy)
    big = torch.full((n + 8,), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    # gy overlaps g without being g
    assert clib.proxtv_PD_TV_vjp_dev(1, y.data_ptr(), np.array([0.3]).ctypes.data, np.array([1.0]).ctypes.data, ns.ctypes.data, 3, 1, 2, big.data_ptr(),
                                     0, big.data_ptr() + 64, 0, 0) == 0
    assert b"overlaps" in clib.proxtv_last_error() and bool((big == 7.0).all())
    # ... and the same call with nothing wrong goes through, also the two-term loop with two terms
    assert go() == 1 and clib.proxtv_last_error() == b""
    assert not bool((gy == 7.0).any()) and not bool((x == 7.0).any()) and not np.any(glam == 7.0)
    assert go(which=0, npen=2) == 1


def test_nothing_at_all(dev, clib):
    torch = dev.torch
    g = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    glam = np.full(2, 7.0)
    lams, dims = np.array([0.3, 0.2]), np.array([1.0, 2.0])
    torch.cuda.synchronize()
    for shape in ((0, 4), (4, 0)):
        ns = np.array(shape, dtype=np.int32)
        for which in (0, 1):
            assert clib.proxtv_PD_TV_vjp_dev(which, 0, lams.ctypes.data, dims.ctypes.data, ns.ctypes.data, 2, 2, 3, 0, 0, g.data_ptr(), glam.ctypes.data, 0) == 1
            assert clib.proxtv_last_error() == b""
    assert bool((g == 7.0).all()) and np.all(glam == 7.0)
    empty = dev.device.colmajor_empty((0, 5))
    gx, gl, y = dev.device.tvgen_vjp(empty, empty.clone(), (0.3, 0.2), (1, 2), 3, need_glam=True, need_y=True)
    assert tuple(gx.shape) == (0, 5) and tuple(y.shape) == (0, 5) and gl.shape == (2,)


# ---- 7. the pool cap ---------------------------------------------------------------------------------------------------------------------
def test_a_tape_beyond_the_pool_cap_is_refused():
    """PROXTV_POOL_CAP_MB is read once per process: a fresh child with a 1 MiB cap asks for the 3 * 7 arrays of a 100 x 100 image."""
    env = dict(os.environ, PROXTV_POOL_CAP_MB="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "pd_vjp_cap_child.py")], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "CAP_CHILD_OK" in r.stdout
