"""The derivative of the general-p TV-Lp fibre prox on the GPU: proxtv_tvpg_fibres_vjp_dev through device.tvp_fibres_vjp, and the autograd
wrapper.  The yardstick is the numpy model of tests/tvp_fibres_vjp_model.py (checked against central differences of the host-built forward
in tests/test_tvp_vjp_host.py) applied to the DEVICE's y, within tm.bar; the autograd test differences the device function itself, within
the bars measured there (tm.FD_BAR)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tvp_fibres_vjp_model as tm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def dev(ptv):
    import torch
    from proxtv_amd import device

    class Dev:
        pass

    d = Dev()
    d.torch, d.device = torch, device
    d.up = lambda a: device.to_colmajor(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda())
    d.down = lambda t: t.cpu().numpy()
    return d


# ---- the device against the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", tm.PS)
def test_device_equals_the_model(dev, p):
    """The grid of the host test, one fibre per call: gx and glam within tm.bar of the model on the device's own forward output."""
    worst, iterative = 0.0, 0
    for n, pp, lam, y, g, o in tm.cases():
        if pp != p:
            continue
        x = dev.device.tvp_fibres(dev.up(y), lam, p, 0)
        gx, glam = dev.device.tvp_fibres_vjp(x, dev.up(g), lam, p, 0, need_glam=True)
        assert glam.shape == () and tuple(gx.shape) == (n,)
        xh = dev.down(x)
        want_gx, want_glam = tm.vjp_1d(xh, g, lam, p)
        bound = tm.bar(xh, g, lam, p)
        ex, el = float(np.max(np.abs(dev.down(gx) - want_gx))), abs(float(glam) - want_glam)
        worst = max(worst, ex / bound, el / bound)
        assert ex <= bound and el <= bound, (n, p, lam, ex, el, bound)
        iterative += int(tm.parts(xh, p)[1] > 0.0)
        if n == 1:
            assert np.array_equal(dev.down(gx), g) and float(glam) == 0.0
    print(f"p {p}: worst ratio to the bar {worst:.2e}, {iterative} iterative fibres")
    assert iterative >= 10


# ---- geometry --------------------------------------------------------------------------------------------------------------------------------
def mixed(shape, dim, seed):
    """Unit-normal data in which, along `dim`, every fifth fibre is constant and every seventh is tiny (the forward answers with its mean):
    adjacent lanes of one wave take different branches."""
    rng = np.random.default_rng(seed)
    x, g = rng.standard_normal(shape), rng.standard_normal(shape)
    xm = np.moveaxis(x, dim, -1)                 # (a view: the edits land in x)
    rows = np.arange(int(np.prod(shape)) // shape[dim])
    idx = np.array(np.unravel_index(rows, xm.shape[:-1])).T
    for r, i in zip(rows, idx):
        if r % 5 == 1:
            xm[tuple(i)] = 0.25 * r
        elif r % 7 == 2:
            xm[tuple(i)] *= 1e-4
    return x, g


def fibre_by_fibre(dev, y, g, lam, p, dim):
    """gx and glam of every fibre through its own 1-D call, assembled like the batch's."""
    torch = dev.torch
    ym, gm = torch.movedim(y, dim, -1), torch.movedim(g, dim, -1)
    gx = torch.empty_like(ym)
    glam = torch.empty(ym.shape[:-1], dtype=torch.float64, device=y.device)
    for idx in np.ndindex(*ym.shape[:-1]):
        a, b = dev.device.tvp_fibres_vjp(ym[idx].contiguous(), gm[idx].contiguous(), lam, p, 0, need_glam=True)
        gx[idx], glam[idx] = a, b
    return torch.movedim(gx, -1, dim), glam


@pytest.mark.parametrize("shape,dim,p", [((37, 70, 3), 0, 1.5), ((37, 70, 3), 1, 3.0), ((37, 70, 3), 2, 1.5), ((9, 130), 0, 3.0),
                                         ((9, 130), 1, 1.5), ((20, 65), 0, 1.5), ((65, 20), 1, 3.0)])
def test_every_fibre_of_a_batch_is_its_own_call(dev, shape, dim, p):
    """Bit for bit, in gx and glam; constant, mean and iterative fibres sit in adjacent lanes; twice and in place: the same bits; and
    with w = 0 every lane copies."""
    torch = dev.torch
    lam = 0.3
    x, g = mixed(shape, dim, 100 + dim)
    y = dev.device.tvp_fibres(dev.up(x), lam, p, dim)
    gd = dev.up(g)
    gx, glam = dev.device.tvp_fibres_vjp(y, gd, lam, p, dim, need_glam=True)
    assert tuple(glam.shape) == tuple(np.delete(shape, dim)) and torch.equal(gd, dev.up(g))
    want_gx, want_glam = fibre_by_fibre(dev, y, gd, lam, p, dim)
    assert torch.equal(gx, want_gx) and torch.equal(glam, want_glam)
    jumps = np.abs(np.diff(np.moveaxis(dev.down(y), dim, -1), axis=-1)).max(axis=-1)
    assert np.any(jumps == 0.0) and np.any(jumps > 0.0)
    assert np.all(dev.down(glam)[jumps == 0.0] == 0.0) and np.all(np.isfinite(dev.down(gx)))
    gx2, glam2 = dev.device.tvp_fibres_vjp(y, gd, lam, p, dim, need_glam=True)
    assert torch.equal(gx, gx2) and torch.equal(glam, glam2)
    h = dev.up(g)
    gx3, glam3 = dev.device.tvp_fibres_vjp(y, h, lam, p, dim, need_glam=True, out=h)
    assert gx3 is h and torch.equal(gx3, gx) and torch.equal(glam3, glam)
    assert torch.equal(dev.device.tvp_fibres_vjp(y, torch.from_numpy(np.ascontiguousarray(g)).cuda(), lam, p, dim), gx)   # (glam = NULL)
    gx0, glam0 = dev.device.tvp_fibres_vjp(y, gd, 0.0, p, dim, need_glam=True)
    assert torch.equal(gx0, gd) and not bool(glam0.any())


@pytest.mark.parametrize("p", [1.5, 3.0])
def test_one_fibre_of_5000_samples(dev, p):
    """One lane walks it, alone (a 1-D array) and as a column of three along dimension 0 (the transposed route): the same bits; and the
    Jacobian is symmetric on it."""
    torch = dev.torch
    n, lam = 5000, 0.5
    rng = np.random.default_rng(50)
    x, g, o = rng.standard_normal((n, 3)), rng.standard_normal((n, 3)), rng.standard_normal(n)
    y = dev.device.tvp_fibres(dev.up(x), lam, p, 0)
    gx, glam = dev.device.tvp_fibres_vjp(y, dev.up(g), lam, p, 0, need_glam=True)
    y1 = y[:, 1].contiguous()
    gx1, glam1 = dev.device.tvp_fibres_vjp(y1, dev.up(g[:, 1]), lam, p, 0, need_glam=True)
    assert torch.equal(gx[:, 1], gx1) and float(glam[1]) == float(glam1) and bool(torch.isfinite(gx).all())
    jo = dev.device.tvp_fibres_vjp(y1, dev.up(o), lam, p, 0)
    lhs, rhs = float(o @ dev.down(gx1)), float(g[:, 1] @ dev.down(jo))
    # ||J|| <= 1: each product is a sum of n terms no larger than max|o| max|g|
    assert abs(lhs - rhs) <= 1e-9 * n * np.abs(o).max() * np.abs(g).max(), (lhs, rhs)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_unwritten(dev, clib):
    torch = dev.torch
    shape = (9, 6)
    rng = np.random.default_rng(8)
    ns = np.array(shape, dtype=np.int32)
    y = dev.device.tvp_fibres(dev.up(rng.standard_normal(shape)), 0.3, 1.5, 0)
    g = dev.up(rng.standard_normal(shape))
    gx, glam = torch.full_like(g, 7.0), torch.full((6,), 7.0, dtype=torch.float64, device=g.device)
    torch.cuda.synchronize()

    def call(yp, gp, gxp, glamp, dim=0, p=1.5, nds=2):
        return clib.proxtv_tvpg_fibres_vjp_dev(yp, gp, gxp, glamp, ns.ctypes.data, nds, dim, 0.3, p, None)

    def refused(r, word):
        err = clib.proxtv_last_error().decode()
        torch.cuda.synchronize()
        assert r == 0 and word in err, (r, err)
        assert bool((gx == 7.0).all()) and bool((glam == 7.0).all())

    for p in (1.0, 2.0, 1.002, 100.0, np.inf):
        refused(call(y.data_ptr(), g.data_ptr(), gx.data_ptr(), glam.data_ptr(), p=p), "p")
    refused(call(y.data_ptr(), g.data_ptr(), gx.data_ptr(), glam.data_ptr(), p=1.0), "proxtv_tv1_fibres_vjp_dev")
    refused(call(y.data_ptr(), g.data_ptr(), gx.data_ptr(), glam.data_ptr(), p=2.0), "proxtv_tv2_fibres_vjp_dev")
    refused(call(0, g.data_ptr(), gx.data_ptr(), glam.data_ptr()), "required")
    refused(call(y.data_ptr(), 0, gx.data_ptr(), glam.data_ptr()), "required")
    refused(call(y.data_ptr(), g.data_ptr(), 0, glam.data_ptr()), "required")
    for dim in (-1, 2):
        refused(call(y.data_ptr(), g.data_ptr(), gx.data_ptr(), glam.data_ptr(), dim=dim), "dimension")
    # overlaps: gx on y, gx shifted into g, glam inside g / y / gx
    big = torch.full((2 * g.numel(),), 7.0, dtype=torch.float64, device=g.device)
    big[:g.numel()] = g.reshape(-1)
    torch.cuda.synchronize()
    assert call(y.data_ptr(), g.data_ptr(), y.data_ptr(), glam.data_ptr()) == 0 and "overlaps" in clib.proxtv_last_error().decode()
    assert call(y.data_ptr(), big.data_ptr(), big.data_ptr() + 8, glam.data_ptr()) == 0 and "overlaps" in clib.proxtv_last_error().decode()
    assert bool((big[g.numel():] == 7.0).all()) and torch.equal(big[:g.numel()], g.reshape(-1))
    refused(call(y.data_ptr(), g.data_ptr(), gx.data_ptr(), g.data_ptr()), "overlaps")
    refused(call(y.data_ptr(), g.data_ptr(), gx.data_ptr(), y.data_ptr() + 16), "overlaps")
    refused(call(y.data_ptr(), g.data_ptr(), gx.data_ptr(), gx.data_ptr()), "overlaps")
    # an empty array: 1, nothing written; glam = NULL and gx == g: served
    ns0 = np.array((0, 6), dtype=np.int32)
    assert clib.proxtv_tvpg_fibres_vjp_dev(0, 0, 0, 0, ns0.ctypes.data, 2, 0, 0.3, 1.5, None) == 1 and clib.proxtv_last_error() == b""
    assert call(y.data_ptr(), g.data_ptr(), gx.data_ptr(), 0) == 1 and clib.proxtv_last_error() == b""
    torch.cuda.synchronize()
    assert torch.equal(gx, dev.device.tvp_fibres_vjp(y, g, 0.3, 1.5, 0)) and bool((glam == 7.0).all())
    h = g.clone()
    assert call(y.data_ptr(), h.data_ptr(), h.data_ptr(), 0) == 1
    torch.cuda.synchronize()
    assert torch.equal(h, gx)
    # the Python surface
    for p, name in ((1, "tv1_fibres_vjp"), (2.0, "tv2_fibres_vjp")):
        with pytest.raises(ValueError, match=name):
            dev.device.tvp_fibres_vjp(y, g, 0.3, p, 0)
    for p in (1.002, 100.0, np.inf):
        with pytest.raises(NotImplementedError):
            dev.device.tvp_fibres_vjp(y, g, 0.3, p, 0)
    with pytest.raises(ValueError):
        dev.device.tvp_fibres_vjp(y, g, 0.3, 1.5, 2)
    with pytest.raises(ValueError):
        dev.device.tvp_fibres_vjp(y, g[:, :3], 0.3, 1.5, 0)


def test_scratch_beyond_the_pool_cap_is_refused():
    """PROXTV_POOL_CAP_MB is read once per process: a fresh child with a 1 MiB cap."""
    env = dict(os.environ, PROXTV_POOL_CAP_MB="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "tvp_fibres_vjp_cap_child.py")], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "CAP_CHILD_OK" in r.stdout


# ---- autograd --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [0, 1])
@pytest.mark.parametrize("p", [1.5, 3.0])
def test_autograd_against_central_differences(dev, p, dim):
    """backward in x and in a 0-d w against central differences (h = 1e-5) through device.tvp_fibres, within the bar the host test
    measured for the arm (tm.FD_BAR); the forward is device.tvp_fibres bit for bit and only y is saved."""
    from proxtv_amd import autograd
    torch = dev.torch
    rng = np.random.default_rng(71)
    shape, lam, h = (24, 18), 0.8, tm.FD_H
    x, c = rng.standard_normal(shape), rng.standard_normal(shape)
    cd = dev.up(c)

    def loss(xa, w):
        return float((cd * dev.device.tvp_fibres(dev.up(xa), w, p, dim)).sum())

    xt = dev.up(x).requires_grad_(True)
    wt = torch.tensor(lam, dtype=torch.float64, requires_grad=True)
    y = autograd.tvp_fibres(xt, wt, p, dim)
    assert torch.equal(y.detach(), dev.device.tvp_fibres(dev.up(x), lam, p, dim))
    saved = y.grad_fn.saved_tensors
    assert len(saved) == 1 and torch.equal(saved[0], y.detach())
    gxt, gwt = torch.autograd.grad((cd * y).sum(), (xt, wt))
    assert gxt.dtype == torch.float64 and gxt.device == xt.device and dev.device._is_colmajor(gxt)
    assert gwt.device == wt.device and gwt.shape == ()
    fd = np.empty(shape)
    for idx in np.ndindex(*shape):
        e = np.zeros(shape)
        e[idx] = h
        fd[idx] = (loss(x + e, lam) - loss(x - e, lam)) / (2 * h)
    ex = float(np.max(np.abs(dev.down(gxt) - fd)))
    ew = abs(float(gwt) - (loss(x, lam + h) - loss(x, lam - h)) / (2 * h))
    print(f"p {p} dim {dim}: |grad x - fd| {ex:.2e}, |grad w - fd| {ew:.2e} (bar {tm.FD_BAR[tm.arm(p)]:.1e})")
    assert ex <= tm.FD_BAR[tm.arm(p)] and ew <= tm.FD_BAR[tm.arm(p)]
    # only x asks: no glam is computed; nothing asks: the plain device call
    xt2 = dev.up(x).requires_grad_(True)
    (cd * autograd.tvp_fibres(xt2, lam, p, dim)).sum().backward()
    assert torch.equal(xt2.grad, gxt)
    assert autograd.tvp_fibres(dev.up(x), lam, p, dim).grad_fn is None


@pytest.mark.parametrize("p", [1, 2])
def test_autograd_p1_and_p2_are_the_exact_solvers(dev, p):
    from proxtv_amd import autograd
    torch = dev.torch
    rng = np.random.default_rng(72)
    x, c = rng.standard_normal((24, 18)), dev.up(rng.standard_normal((24, 18)))
    own = autograd.tv1_fibres if p == 1 else autograd.tv2_fibres
    for dim in (0, 1):
        res = []
        for fn in (lambda xt, wt: autograd.tvp_fibres(xt, wt, p, dim), lambda xt, wt: own(xt, wt, dim)):
            xt = dev.up(x).requires_grad_(True)
            wt = torch.tensor(0.8, dtype=torch.float64, requires_grad=True)
            y = fn(xt, wt)
            res.append((y.detach(),) + torch.autograd.grad((c * y).sum(), (xt, wt)))
        for a, b in zip(*res):
            assert torch.equal(a, b)


def test_solver_derivatives_still_refuse_a_general_p(ptv, dev):
    from proxtv_amd import autograd
    img = dev.up(np.random.default_rng(2).standard_normal((8, 6)))
    before = ptv.general_p(False)
    try:
        for on in (True, False):
            ptv.general_p(on)
            with pytest.raises(NotImplementedError):
                dev.device.dr2_vjp(img, img, 0.3, p_col=1.5)
            with pytest.raises(NotImplementedError):
                dev.device.tvgen_vjp(img, img, [0.3, 0.3], [1, 2], 3, ps=[1.5, 1])
            with pytest.raises(NotImplementedError):
                autograd.tvp_2d(img, 0.3, 0.3, 1.5, 1)
    finally:
        ptv.general_p(before)
