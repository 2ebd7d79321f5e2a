"""The derivative of the 2-D Douglas-Rachford TV-L1 solves on the GPU: proxtv_DR2_TV_vjp_dev through device.dr2_vjp, and the autograd
wrappers tv1_2d / tv1w_2d / tv1_2d_batch.  Yardsticks: the numpy model of tests/dr_vjp_model.py (checked against central differences
in tests/test_dr_vjp_model.py), central differences of the fused device solves themselves, and the recurrence composed in torch from
autograd.tv1_fibres.  Tolerances of the model comparisons: dr_vjp_model.sweep_scale."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import dr_vjp_model as dm
import vjp_model as vm
from conftest import REL_TOL, rel_err

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# (seed, shape, lambda, maxit, weighted): the cases of the CPU test, and two shapes with more than one chunk of 16 / wave of 64 fibres
MODEL_CASES = tuple(c + (False,) for c in dm.UNIFORM_CASES) + tuple(c + (True,) for c in dm.WEIGHTED_CASES) + \
    ((21, (65, 17), 0.3, 35, False), (22, (17, 65), 0.3, 35, False), (21, (65, 17), 0.3, 35, True), (22, (17, 65), 0.3, 35, True))


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
def model(seed, shape, lam, maxit, weighted):
    """One case, once: inputs, the model's forward result and gradients (shared by the tests; nobody writes into them)."""
    from oracle import cpu
    U, g, W1m, W2m = dm.draw(seed, shape, lam, weighted)
    W1, W2 = (0.0, 0.0) if weighted else (lam, dm.ROW_RATIO * lam)
    out, tape = dm.forward(cpu.oracle(), U, W1, W2, maxit, W1m, W2m)
    dm.assert_tape_unambiguous(tape)
    gU, gW1, gW2 = dm.reverse(tape, g)
    for a in (U, g, out, gU, gW1, gW2):
        a.setflags(write=False)
    return dict(U=U, g=g, W1=W1, W2=W2, W1m=W1m, W2m=W2m, out=out, gU=gU, gW1=gW1, gW2=gW2, maxit=maxit, scale=dm.sweep_scale(shape, maxit, g))


def call(dev, m, **kw):
    """device.dr2_vjp on a case of model(); everything asked for unless told otherwise."""
    kw.setdefault("need_gw", True)
    kw.setdefault("need_y", True)
    wc, wr = (None, None) if m["W1m"] is None else (dev.up(m["W1m"]), dev.up(m["W2m"]))
    return dev.device.dr2_vjp(dev.up(m["U"]), dev.up(m["g"]), m["W1"], m["W2"], m["maxit"], weights_col=wc, weights_row=wr, **kw)


def worst(got, want):
    return float(np.max(np.abs(got - want))) if want.size else 0.0


# ---- 1. against the numpy model --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,shape,lam,maxit,weighted", MODEL_CASES)
def test_against_the_model(dev, seed, shape, lam, maxit, weighted):
    m = model(seed, shape, lam, maxit, weighted)
    gx, gwc, gwr, glam, y = call(dev, m)
    scale = m["scale"]
    ex, e1, e2 = worst(dev.down(gx), m["gU"]), worst(dev.down(gwc), m["gW1"]), worst(dev.down(gwr), m["gW2"])
    l1, l2 = abs(glam[0] - m["gW1"].sum()), abs(glam[1] - m["gW2"].sum())
    print(f"seed {seed} {shape} lambda {lam} maxit {maxit} weighted {weighted}: |gU - model| {ex:.2e} (bar {scale:.2e}), |gW1| {e1:.2e}, "
          f"|gW2| {e2:.2e} (bar {2 * scale:.2e}), |glam| {l1:.2e} {l2:.2e}")
    assert tuple(gwc.shape) == (shape[0] - 1, shape[1]) and tuple(gwr.shape) == (shape[0], shape[1] - 1) and glam.shape == (2,)
    assert ex <= scale
    assert e1 <= 2 * scale and e2 <= 2 * scale
    assert l1 <= 2 * scale * max(m["gW1"].size, 1) and l2 <= 2 * scale * max(m["gW2"].size, 1)
    assert rel_err(dev.down(y), m["out"]) <= REL_TOL


# ---- 2. against central differences of the fused solves -------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,shape,lam,maxit,weighted", [c for c in MODEL_CASES if c[0] in (1, 2, 4, 5, 8, 11)])
def test_against_central_differences_of_the_device_solves(dev, seed, shape, lam, maxit, weighted):
    m = model(seed, shape, lam, maxit, weighted)
    cd = dev.up(m["g"])
    h = vm.FD_H
    gx, gwc, gwr, glam, _ = call(dev, m)
    if weighted:
        def loss(u, w1=m["W1m"], w2=m["W2m"]):
            return float((cd * dev.device.tv1w_2d(dev.up(u), dev.up(w1), dev.up(w2), maxit)[0]).sum())
        ep = max(worst(dev.down(gwc), vm.central_x(lambda w: loss(m["U"], w1=w), m["W1m"].copy())),
                 worst(dev.down(gwr), vm.central_x(lambda w: loss(m["U"], w2=w), m["W2m"].copy())))
    else:
        def loss(u, w1=m["W1"], w2=m["W2"]):
            return float((cd * dev.device.tv1_2d(dev.up(u), w1, maxit, w_row=w2)[0]).sum())
        ep = max(abs(glam[0] - (loss(m["U"], w1=m["W1"] + h) - loss(m["U"], w1=m["W1"] - h)) / (2 * h)),
                 abs(glam[1] - (loss(m["U"], w2=m["W2"] + h) - loss(m["U"], w2=m["W2"] - h)) / (2 * h)))
    ex = worst(dev.down(gx), vm.central_x(loss, m["U"].copy()))
    print(f"seed {seed} {shape} weighted {weighted}: |gU - fd| {ex:.2e}, |penalties - fd| {ep:.2e} (bar {vm.FD_TOL:.0e})")
    assert ex <= vm.FD_TOL and ep <= vm.FD_TOL


# ---- 3. against the recurrence composed in torch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_against_the_torch_composition(dev, weighted):
    """(130, 70): several chunks of 16 samples and more than one wave of 64 fibres in both geometries."""
    from proxtv_amd import autograd
    torch = dev.torch
    m = model(31, (130, 70), 0.3, 35, weighted)
    U = dev.up(m["U"]).requires_grad_(True)
    if weighted:
        pens = [dev.up(m["W1m"]).requires_grad_(True), dev.up(m["W2m"]).requires_grad_(True)]
        out = dm.compose(torch, autograd, U, 0.0, 0.0, m["maxit"], pens[0], pens[1])
    else:
        pens = [torch.tensor(w, dtype=torch.float64, device="cuda", requires_grad=True) for w in (m["W1"], m["W2"])]
        out = dm.compose(torch, autograd, U, pens[0], pens[1], m["maxit"])
    (dev.up(m["g"]) * out).sum().backward()
    gx, gwc, gwr, glam, y = call(dev, m)
    scale = m["scale"]
    ex = worst(dev.down(gx), dev.down(U.grad))
    if weighted:
        e1, e2 = worst(dev.down(gwc), dev.down(pens[0].grad)), worst(dev.down(gwr), dev.down(pens[1].grad))
    else:
        e1, e2 = abs(glam[0] - float(pens[0].grad)) / m["gW1"].size, abs(glam[1] - float(pens[1].grad)) / m["gW2"].size
    ey = worst(dev.down(y), dev.down(out.detach()))
    print(f"weighted {weighted}: |gU - composition| {ex:.2e} (bar {scale:.2e}), penalties {e1:.2e} {e2:.2e} (bar {2 * scale:.2e}), forward {ey:.2e}")
    assert ex <= scale and e1 <= 2 * scale and e2 <= 2 * scale
    assert worst(dev.down(gx), m["gU"]) <= scale


# ---- 4. the forward result ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,shape,weighted", [(21, (65, 17), False), (21, (65, 17), True), (31, (130, 70), False), (4, (1, 9), False),
                                                 (5, (8, 1), False)])
def test_forward_result(dev, oracle, seed, shape, weighted):
    m = model(seed, shape, 0.3 if seed in (21, 31) else 0.5, 35, weighted)
    _, _, _, _, y = call(dev, m, need_gw=False)
    if weighted:
        want = oracle.dr2w(m["U"], m["W1m"], m["W2m"])[0]
        fused = dev.device.tv1w_2d(dev.up(m["U"]), dev.up(m["W1m"]), dev.up(m["W2m"]))[0]
    else:
        want = oracle.dr2(m["U"], m["W1"], m["W2"])[0]
        fused = dev.device.tv1_2d(dev.up(m["U"]), m["W1"], w_row=m["W2"])[0]
    print(f"seed {seed} {shape} weighted {weighted}: relative error vs oracle {rel_err(dev.down(y), want):.2e}, "
          f"|s - proxtv_DR2_TV_dev| {worst(dev.down(y), dev.down(fused)):.2e}")
    assert rel_err(dev.down(y), want) <= REL_TOL


# ---- 5. reproducibility ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_same_bits_every_call_and_in_place(dev, clib, weighted):
    torch = dev.torch
    m = model(31, (130, 70), 0.3, 35, weighted)
    first, again = call(dev, m), call(dev, m)
    for a, b in zip(first, again):
        assert torch.equal(a, b) if isinstance(a, torch.Tensor) else np.array_equal(a, b)
    # gU is g: the C-ABI directly (device.dr2_vjp always returns a fresh gx)
    M, N = m["U"].shape
    U, g = dev.up(m["U"]), dev.up(m["g"])
    wc, wr = (None, None) if not weighted else (dev.up(m["W1m"]), dev.up(m["W2m"]))
    gw1, gw2 = dev.device.colmajor_empty((M - 1, N)), dev.device.colmajor_empty((M, N - 1))
    glam = np.zeros(2)
    torch.cuda.synchronize()
    assert clib.proxtv_DR2_TV_vjp_dev(M, N, 1, U.data_ptr(), m["W1"], m["W2"], wc.data_ptr() if weighted else 0, wr.data_ptr() if weighted else 0,
                                      g.data_ptr(), 0, g.data_ptr(), gw1.data_ptr(), gw2.data_ptr(), glam.ctypes.data, 35, 0) == 1
    assert torch.equal(g, first[0]) and torch.equal(gw1, first[1]) and torch.equal(gw2, first[2]) and np.array_equal(glam, first[3])


# ---- 6. batch ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_batch_images_have_the_bits_of_their_own_calls(dev, weighted):
    torch = dev.torch
    ms = [model(seed, (33, 20), 0.3, 35, weighted) for seed in (41, 42, 43)]
    stack = lambda key: dev.up(np.stack([m[key] for m in ms], axis=2))   # noqa: E731
    wc, wr = (None, None) if not weighted else (stack("W1m"), stack("W2m"))
    gx, gwc, gwr, glam, y = dev.device.dr2_vjp(stack("U"), stack("g"), ms[0]["W1"], ms[0]["W2"], 35, weights_col=wc, weights_row=wr,
                                               need_gw=True, need_y=True)
    assert glam.shape == (3, 2) and tuple(gwc.shape) == (32, 20, 3) and tuple(gwr.shape) == (33, 19, 3)
    for b, m in enumerate(ms):
        one = call(dev, m)
        for name, got, want in zip(("gU", "gW1", "gW2", "glam", "s"), (gx, gwc, gwr, glam, y), one):
            if name == "glam":
                assert np.array_equal(got[b], want), (b, name)
            else:
                assert torch.equal(got[:, :, b], want), (b, name)
        assert worst(dev.down(gx[:, :, b]), m["gU"]) <= m["scale"]


# ---- 7. autograd ---------------------------------------------------------------------------------------------------------------------------
def test_autograd_uniform(dev):
    from proxtv_amd import autograd
    torch = dev.torch
    m = model(2, (12, 5), 0.8, 35, False)
    x = dev.up(m["U"])
    assert autograd.tv1_2d(x, m["W1"], w_row=m["W2"]).grad_fn is None
    with torch.no_grad():
        assert autograd.tv1_2d(x.clone().requires_grad_(True), m["W1"]).grad_fn is None
    xt = x.clone().requires_grad_(True)
    w1 = torch.tensor(m["W1"], dtype=torch.float64, requires_grad=True)                    # on the CPU: its gradient comes back there
    w2 = torch.tensor(m["W2"], dtype=torch.float64, device="cuda", requires_grad=True)
    y = autograd.tv1_2d(xt, w1, w_row=w2)
    assert y.grad_fn is not None and torch.equal(y.detach(), dev.device.tv1_2d(x, m["W1"], w_row=m["W2"])[0])
    (dev.up(m["g"]) * y).sum().backward()
    assert xt.grad.dtype == torch.float64 and xt.grad.device == xt.device and dev.device._is_colmajor(xt.grad)
    assert w1.grad.device == w1.device and w2.grad.device == w2.device and w1.grad.shape == () and w1.grad.dtype == torch.float64
    scale = m["scale"]
    assert worst(dev.down(xt.grad), m["gU"]) <= scale
    assert abs(float(w1.grad) - m["gW1"].sum()) <= 2 * scale * m["gW1"].size and abs(float(w2.grad) - m["gW2"].sum()) <= 2 * scale * m["gW2"].size
    # one tensor for both directions receives the sum; only the penalty asks
    mm = model(6, (2, 2), 0.4, 35, False)
    w = torch.tensor(0.4, dtype=torch.float64, device="cuda", requires_grad=True)
    yy = autograd.tv1_2d(dev.up(mm["U"]), w, w_row=dm.ROW_RATIO * 0.4)
    (dev.up(mm["g"]) * yy).sum().backward()
    assert abs(float(w.grad) - mm["gW1"].sum()) <= 2 * mm["scale"] * mm["gW1"].size
    with pytest.raises(ValueError):
        autograd.tv1_2d(xt, torch.tensor([0.3], dtype=torch.float64))


def test_autograd_weight_maps(dev):
    from proxtv_amd import autograd
    torch = dev.torch
    m = model(11, (9, 7), 0.3, 35, True)
    x, wc, wr = dev.up(m["U"]), dev.up(m["W1m"]), dev.up(m["W2m"])
    assert autograd.tv1w_2d(x, wc, wr).grad_fn is None
    xt, wct, wrt = (t.clone().requires_grad_(True) for t in (x, wc, wr))
    y = autograd.tv1w_2d(xt, wct, wrt)
    assert y.grad_fn is not None and torch.equal(y.detach(), dev.device.tv1w_2d(x, wc, wr)[0])
    (dev.up(m["g"]) * y).sum().backward()
    for t in (xt, wct, wrt):
        assert t.grad.dtype == torch.float64 and t.grad.device == t.device and dev.device._is_colmajor(t.grad) and t.grad.shape == t.shape
    assert worst(dev.down(xt.grad), m["gU"]) <= m["scale"]
    assert worst(dev.down(wct.grad), m["gW1"]) <= 2 * m["scale"] and worst(dev.down(wrt.grad), m["gW2"]) <= 2 * m["scale"]


def test_autograd_batch(dev):
    from proxtv_amd import autograd
    torch = dev.torch
    lam = 0.3
    Us = [dm.draw(seed, (33, 20), lam)[0] for seed in (41, 42, 43)]
    gs = [dm.draw(seed, (33, 20), lam)[1] for seed in (41, 42, 43)]
    xs = dev.up(np.stack(Us, axis=2))
    assert autograd.tv1_2d_batch(xs, lam).grad_fn is None
    xt = xs.clone().requires_grad_(True)
    w = torch.tensor(lam, dtype=torch.float64, device="cuda", requires_grad=True)
    y = autograd.tv1_2d_batch(xt, w)
    assert y.grad_fn is not None and torch.equal(y.detach(), dev.device.tv1_2d_batch(xs, lam)[0])
    (dev.up(np.stack(gs, axis=2)) * y).sum().backward()
    assert xt.grad.dtype == torch.float64 and xt.grad.device == xt.device and dev.device._is_colmajor(xt.grad) and w.grad.device == w.device
    # expected values: the model image by image, both penalties equal here (tv1_2d_batch has one w)
    from oracle import cpu
    want_w = 0.0
    for b in range(3):
        out, tape = dm.forward(cpu.oracle(), Us[b], lam, lam, 35)
        dm.assert_tape_unambiguous(tape)
        gU, gW1, gW2 = dm.reverse(tape, gs[b])
        scale = dm.sweep_scale((33, 20), 35, gs[b])
        assert worst(dev.down(xt.grad[:, :, b]), gU) <= scale
        want_w += gW1.sum() + gW2.sum()
    assert abs(float(w.grad) - want_w) <= 2 * scale * 3 * (gW1.size + gW2.size)


# ---- 8. bad arguments ----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments(dev, clib):
    torch = dev.torch
    M, N = 6, 4
    U, g = dev.up(np.arange(24.0).reshape(M, N)), dev.up(np.ones((M, N)))
    w1, w2 = dev.up(np.full((M - 1, N), 0.5)), dev.up(np.full((M, N - 1), 0.5))
    for bad in (dict(weights_col=w1), dict(weights_row=w2), dict(weights_col=w2, weights_row=w1),
                dict(weights_col=w1.float(), weights_row=w2)):
        with pytest.raises(ValueError):
            dev.device.dr2_vjp(U, g, 0.5, **bad)
    with pytest.raises(ValueError):
        dev.device.dr2_vjp(U, dev.up(np.ones((M, N + 1))), 0.5)
    with pytest.raises(ValueError):
        dev.device.dr2_vjp(U, g.float(), 0.5)
    with pytest.raises(ValueError):
        dev.device.dr2_vjp(dev.up(np.ones(5)), dev.up(np.ones(5)), 0.5)
    # the C-ABI itself: refused, proxtv_last_error set, nothing written
    gU, s = torch.full_like(g, 7.0), torch.full_like(g, 7.0)
    gw1, gw2 = torch.full_like(w1, 7.0), torch.full_like(w2, 7.0)
    glam = np.full(2, 7.0)
    torch.cuda.synchronize()     # (the C calls below run on the library's own stream)

    def refused(why, unary=U, W1m=None, W2m=None, cot=g, out=s, gu=gU):
        p = lambda t: 0 if t is None else t.data_ptr()   # noqa: E731
        rc = clib.proxtv_DR2_TV_vjp_dev(M, N, 1, p(unary), 0.5, 0.5, p(W1m), p(W2m), p(cot), p(out), p(gu), gw1.data_ptr(), gw2.data_ptr(),
                                        glam.ctypes.data, 0, 0)
        assert rc == 0 and why in clib.proxtv_last_error(), (why, clib.proxtv_last_error())
        for t in (gU, s, gw1, gw2):
            assert bool((t == 7.0).all()), why
        assert np.all(glam == 7.0), why
        assert bool((U == dev.up(np.arange(24.0).reshape(M, N))).all()) and bool((g == 1.0).all())

    refused(b"pairs", W1m=w1)
    refused(b"pairs", W2m=w2)
    refused(b"overlaps", out=U)
    refused(b"overlaps", gu=U)
    refused(b"overlaps", out=g)
    refused(b"required", gu=None)
    refused(b"required", cot=None)
    # ... and the same call with nothing wrong goes through
    assert clib.proxtv_DR2_TV_vjp_dev(M, N, 1, U.data_ptr(), 0.5, 0.5, 0, 0, g.data_ptr(), s.data_ptr(), gU.data_ptr(), gw1.data_ptr(),
                                      gw2.data_ptr(), glam.ctypes.data, 0, 0) == 1
    assert not bool((gU == 7.0).any()) and not bool((s == 7.0).any()) and not np.any(glam == 7.0)


def test_a_tape_beyond_the_pool_cap_is_refused():
    """PROXTV_POOL_CAP_MB is read once per process: a fresh child with a 1 MiB cap asks for a 72-array tape of a 100 x 100 image (5.76 MB)."""
    env = dict(os.environ, PROXTV_POOL_CAP_MB="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "dr_vjp_cap_child.py")], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "CAP_CHILD_OK" in r.stdout


# ---- 9. one iteration, and nothing at all -------------------------------------------------------------------------------------------------
def test_empty_arrays(dev, clib):
    torch = dev.torch
    g = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    glam = np.full(2, 7.0)
    torch.cuda.synchronize()
    for M, N, B in ((0, 4, 1), (4, 0, 1), (2, 2, 0)):
        assert clib.proxtv_DR2_TV_vjp_dev(M, N, B, g.data_ptr(), 0.5, 0.5, 0, 0, g.data_ptr(), 0, g.data_ptr(), 0, 0, glam.ctypes.data, 0, 0) == 1
        assert clib.proxtv_last_error() == b""
    assert bool((g == 7.0).all()) and np.all(glam == 7.0)
    gx, gwc, gwr, glam, y = dev.device.dr2_vjp(dev.device.colmajor_empty((0, 5)), dev.device.colmajor_empty((0, 5)), 0.5, need_gw=True, need_y=True)
    assert tuple(gx.shape) == (0, 5) and tuple(y.shape) == (0, 5)


def test_one_iteration_is_the_default_when_asked_for_nothing(dev):
    """max_iters = 1 is in MODEL_CASES (seed 8); max_iters <= 0 means 35."""
    m = model(1, (9, 7), 0.3, 35, False)
    a = call(dev, m)
    b = dev.device.dr2_vjp(dev.up(m["U"]), dev.up(m["g"]), m["W1"], m["W2"], 0, need_gw=True, need_y=True)
    c = dev.device.dr2_vjp(dev.up(m["U"]), dev.up(m["g"]), m["W1"], m["W2"], -3, need_gw=True, need_y=True)
    for x, y, z in zip(a, b, c):
        same = dev.torch.equal if isinstance(x, dev.torch.Tensor) else np.array_equal
        assert same(x, y) and same(x, z)
    one = dev.device.dr2_vjp(dev.up(m["U"]), dev.up(m["g"]), m["W1"], m["W2"], 1)[0]
    assert worst(dev.down(one), dev.down(a[0])) > 1e-6     # (and one iteration is not thirty-five)
