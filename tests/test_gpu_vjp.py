"""The derivative of the TV-L1 fibre prox on the GPU: proxtv_tv1_fibres_vjp_dev through device.tv1_fibres_vjp, and the autograd
wrapper.  The yardstick is the numpy model of tests/vjp_model.py (checked against central differences of the CPU oracle in
tests/test_vjp_host.py) applied to the DEVICE's y, within the certifier's rounding rule; the autograd tests difference the device
function itself."""
import numpy as np
import pytest

import vjp_model as vm

pytestmark = pytest.mark.gpu

# the kernels cut fibres into chunks of 16 samples and resolve 64 chunks per trip: each boundary and its neighbours, and one
# fibre long enough for many trips
LENGTHS_1D = vm.LENGTHS + (15, 16, 17, 1023, 1024, 1025, 20011)


@pytest.fixture(scope="module")
def dev(ptv):
    import torch
    from proxtv_amd import device

    class Dev:
        pass

    d = Dev()
    d.torch, d.device = torch, device
    d.up = lambda a: device.to_colmajor(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    d.down = lambda t: t.cpu().numpy()
    return d


def oracle_prox(oracle, x, lam, dim, weights=None):
    """The CPU oracle fibre by fibre along `dim` (what the precondition of every test is checked on)."""
    xm = np.moveaxis(x, dim, -1)
    wm = None if weights is None else np.moveaxis(weights, dim, -1)
    out = np.empty(xm.shape)
    for idx in np.ndindex(*xm.shape[:-1]):
        out[idx] = oracle.tv1_hybrid(xm[idx], lam) if wm is None else (oracle.tv1_weighted(xm[idx], wm[idx]) if xm.shape[-1] > 1 else xm[idx])
    return np.moveaxis(out, -1, dim)


def check_against_model(dev, y_dev, g, dim, what):
    """gx, gw, nseg of one device call against the model on the device's own y; returns the device results."""
    gx, gw, nseg = dev.device.tv1_fibres_vjp(y_dev, dev.up(g), dim, need_gw=True, need_nseg=True)
    y = dev.down(y_dev)
    want_gx, want_gw, want_nseg = vm.vjp_nd(y, g, dim)
    bound = vm.rounding_bound(y.shape[dim], g)
    ex = float(np.max(np.abs(dev.down(gx) - want_gx)))
    ew = float(np.max(np.abs(dev.down(gw) - want_gw))) if want_gw.size else 0.0
    print(f"{what}: |gx - model| {ex:.2e}, |gw - model| {ew:.2e}, bound {bound:.2e}")
    assert ex <= bound, what
    assert ew <= 2 * bound, what
    assert np.array_equal(dev.down(nseg).ravel(order="F"), want_nseg), what
    assert tuple(gw.shape) == tuple(s - (i == dim) for i, s in enumerate(y.shape)) and tuple(nseg.shape) == tuple(np.delete(y.shape, dim))
    return gx, gw, nseg


# ---- (c) 1-D signals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_signals_against_the_model(dev, oracle, weighted):
    rng = np.random.default_rng(2026)
    for n in LENGTHS_1D:
        for lam in vm.LAMBDAS:
            x, c = rng.standard_normal(n), rng.standard_normal(n)
            w = lam * rng.uniform(0.5, 1.5, max(n - 1, 0))
            if weighted and n < 2:
                continue
            vm.assert_unambiguous(oracle.tv1_weighted(x, w) if weighted else oracle.tv1_hybrid(x, lam))
            y = dev.device.tv1_fibres(dev.up(x), lam, 0, weights=dev.up(w) if weighted else None)
            check_against_model(dev, y, c, 0, f"n {n} lambda {lam} weighted {weighted}")


def test_degenerate_penalties(dev, oracle):
    """lambda = 0: every sample its own segment, gx == g exactly.  lambda = 1e6: one segment, gx the fibre's mean, gw == 0."""
    rng = np.random.default_rng(5)
    for n in (1, 2, 17, 300, 1025):
        x, c = rng.standard_normal(n), rng.standard_normal(n)
        vm.assert_unambiguous(oracle.tv1_hybrid(x, 0.0))
        vm.assert_unambiguous(oracle.tv1_hybrid(x, 1e6))
        gx, gw, nseg = dev.device.tv1_fibres_vjp(dev.device.tv1_fibres(dev.up(x), 0.0, 0), dev.up(c), 0, need_gw=True, need_nseg=True)
        assert np.array_equal(dev.down(gx), c) and int(nseg) == n
        gx, gw, nseg = dev.device.tv1_fibres_vjp(dev.device.tv1_fibres(dev.up(x), 1e6, 0), dev.up(c), 0, need_gw=True, need_nseg=True)
        gx = dev.down(gx)
        assert int(nseg) == 1 and np.all(dev.down(gw) == 0.0) and np.all(gx == gx[0])
        assert abs(gx[0] - c.mean()) <= vm.rounding_bound(n, c)


# ---- (d) arrays: both geometries, unit extents, fibre counts that are no multiple of 64 ---------------------------------------------
@pytest.mark.parametrize("shape,dim", [((150, 70, 5), 0), ((150, 70, 5), 1), ((150, 70, 5), 2), ((1, 40), 0), ((1, 40), 1), ((40, 1), 0),
                                       ((40, 1), 1)])
def test_arrays_in_place_and_reproducible(dev, oracle, shape, dim):
    rng = np.random.default_rng(300 + dim)   # (seeds for which the precondition below holds: it is an assert, not a skip)
    x, c = rng.standard_normal(shape), rng.standard_normal(shape)
    lam = 0.8
    vm.assert_unambiguous(oracle_prox(oracle, x, lam, dim), axis=dim)
    y = dev.device.tv1_fibres(dev.up(x), lam, dim)
    gx, gw, nseg = check_against_model(dev, y, c, dim, f"shape {shape} dim {dim}")
    # twice: the same bits
    gx2, gw2, nseg2 = dev.device.tv1_fibres_vjp(y, dev.up(c), dim, need_gw=True, need_nseg=True)
    assert dev.torch.equal(gx, gx2) and dev.torch.equal(gw, gw2) and dev.torch.equal(nseg, nseg2)
    # in place: gx is g
    g = dev.up(c)
    gx3, gw3, _ = dev.device.tv1_fibres_vjp(y, g, dim, need_gw=True, out=g)
    assert gx3 is g and dev.torch.equal(gx3, gx) and dev.torch.equal(gw3, gw)
    # a cotangent in another layout is copied, not rejected; the segment counts alone
    gx4, _, _ = dev.device.tv1_fibres_vjp(y, dev.torch.from_numpy(np.ascontiguousarray(c)).cuda(), dim)
    assert dev.torch.equal(gx4, gx)
    assert dev.torch.equal(dev.device.tv1_fibres_dof(y, dim), nseg)


def test_weighted_array(dev, oracle):
    rng = np.random.default_rng(41)
    shape = (70, 33)
    for dim in (0, 1):
        x, c = rng.standard_normal(shape), rng.standard_normal(shape)
        wshape = tuple(s - (i == dim) for i, s in enumerate(shape))
        w = 0.8 * rng.uniform(0.5, 1.5, wshape)
        vm.assert_unambiguous(oracle_prox(oracle, x, 0.0, dim, w), axis=dim)
        y = dev.device.tv1_fibres(dev.up(x), 0.0, dim, weights=dev.up(w))
        check_against_model(dev, y, c, dim, f"weighted {shape} dim {dim}")


# ---- (e) autograd -----------------------------------------------------------------------------------------------------------------------
def _fd(f, a):
    """Central differences (h = 1e-5) of the scalar device function f in every entry of the numpy array a."""
    return vm.central_x(f, np.ascontiguousarray(a).copy())


@pytest.mark.parametrize("dim", [0, 1])
def test_autograd_against_central_differences(dev, oracle, dim):
    from proxtv_amd import autograd
    torch = dev.torch
    rng = np.random.default_rng(51 + dim)
    shape = (12, 5)
    x, c = rng.standard_normal(shape), rng.standard_normal(shape)
    lam = 0.8
    wshape = tuple(s - (i == dim) for i, s in enumerate(shape))
    wts = lam * rng.uniform(0.5, 1.5, wshape)
    cd = dev.up(c)
    h = vm.FD_H
    vm.assert_unambiguous(oracle_prox(oracle, x, lam, dim), axis=dim)
    vm.assert_unambiguous(oracle_prox(oracle, x, 0.0, dim, wts), axis=dim)

    def loss(xa, w, weights):
        y = dev.device.tv1_fibres(dev.up(xa), w, dim, weights=None if weights is None else dev.up(weights))
        return float((cd * y).sum())

    # uniform penalty: x and the scalar w (a 0-d float64 tensor on the CPU: its gradient comes back there)
    xt = dev.up(x).requires_grad_(True)
    wt = torch.tensor(lam, dtype=torch.float64, requires_grad=True)
    (cd * autograd.tv1_fibres(xt, wt, dim)).sum().backward()
    assert xt.grad.dtype == torch.float64 and xt.grad.device == xt.device and dev.device._is_colmajor(xt.grad)
    assert wt.grad.device == wt.device and wt.grad.shape == ()
    ex = float(np.max(np.abs(dev.down(xt.grad) - _fd(lambda a: loss(a, lam, None), x))))
    ew = abs(float(wt.grad) - (loss(x, lam + h, None) - loss(x, lam - h, None)) / (2 * h))
    print(f"dim {dim}: |grad x - fd| {ex:.2e}, |grad w - fd| {ew:.2e}")
    assert ex <= vm.FD_TOL and ew <= vm.FD_TOL
    # per-edge weights: x and the weights
    xt = dev.up(x).requires_grad_(True)
    wd = dev.up(wts).requires_grad_(True)
    (cd * autograd.tv1_fibres(xt, 0.0, dim, weights=wd)).sum().backward()
    ex = float(np.max(np.abs(dev.down(xt.grad) - _fd(lambda a: loss(a, 0.0, wts), x))))
    ewt = float(np.max(np.abs(dev.down(wd.grad) - _fd(lambda ww: loss(x, 0.0, ww), wts))))
    print(f"dim {dim} weighted: |grad x - fd| {ex:.2e}, |grad weights - fd| {ewt:.2e}")
    assert ex <= vm.FD_TOL and ewt <= vm.FD_TOL


def test_autograd_composition(dev, oracle):
    """tv1_fibres(tv1_fibres(x, w, 0), w, 1): what a user composes a 2-D scheme from."""
    from proxtv_amd import autograd
    torch = dev.torch
    rng = np.random.default_rng(61)
    x, c = rng.standard_normal((9, 7)), rng.standard_normal((9, 7))
    lam, h = 0.3, vm.FD_H
    cd = dev.up(c)
    inner = oracle_prox(oracle, x, lam, 0)
    vm.assert_unambiguous(inner, axis=0)
    vm.assert_unambiguous(oracle_prox(oracle, inner, lam, 1), axis=1)

    def loss(xa, w):
        return float((cd * dev.device.tv1_fibres(dev.device.tv1_fibres(dev.up(xa), w, 0), w, 1)).sum())

    xt = dev.up(x).requires_grad_(True)
    wt = torch.tensor(lam, dtype=torch.float64, device="cuda", requires_grad=True)
    (cd * autograd.tv1_fibres(autograd.tv1_fibres(xt, wt, 0), wt, 1)).sum().backward()
    assert xt.grad.dtype == torch.float64 and xt.grad.device == xt.device and dev.device._is_colmajor(xt.grad)
    assert wt.grad.device == wt.device
    ex = float(np.max(np.abs(dev.down(xt.grad) - _fd(lambda a: loss(a, lam), x))))
    ew = abs(float(wt.grad) - (loss(x, lam + h) - loss(x, lam - h)) / (2 * h))
    print(f"composition: |grad x - fd| {ex:.2e}, |grad w - fd| {ew:.2e}")
    assert ex <= vm.FD_TOL and ew <= vm.FD_TOL


def test_autograd_costs_nothing_when_nothing_asks(dev):
    from proxtv_amd import autograd
    torch = dev.torch
    x = dev.up(np.random.default_rng(3).standard_normal((12, 5)))
    y = autograd.tv1_fibres(x, 0.5, 0)
    assert y.grad_fn is None and not y.requires_grad and torch.equal(y, dev.device.tv1_fibres(x, 0.5, 0))
    with torch.no_grad():
        assert autograd.tv1_fibres(x.clone().requires_grad_(True), 0.5, 0).grad_fn is None
    assert autograd.tv1_fibres(x.clone().requires_grad_(True), 0.5, 0).grad_fn is not None


# ---- (f) bad arguments --------------------------------------------------------------------------------------------------------------------
def test_bad_arguments(dev, clib):
    torch = dev.torch
    y = dev.up(np.zeros((6, 4)))
    g = dev.up(np.ones((6, 4)))
    for dim in (-1, 2):
        with pytest.raises(ValueError):
            dev.device.tv1_fibres_vjp(y, g, dim)
        with pytest.raises(ValueError):
            dev.device.tv1_fibres_dof(y, dim)
    with pytest.raises(ValueError):
        dev.device.tv1_fibres_vjp(y, dev.up(np.ones((6, 3))), 0)
    with pytest.raises(ValueError):
        dev.device.tv1_fibres_vjp(y, g.float(), 0)
    with pytest.raises(ValueError):
        dev.device.tv1_fibres_vjp(y, g, 0, out=dev.up(np.ones((4, 6))))
    # the C-ABI itself: a dimension out of range is refused, nothing is written
    ns = np.array([6, 4], dtype=np.int32)
    out = torch.full_like(g, 7.0)
    torch.cuda.synchronize()     # (the C calls below run on the library's own stream)
    assert clib.proxtv_tv1_fibres_vjp_dev(y.data_ptr(), g.data_ptr(), out.data_ptr(), 0, 0, ns.ctypes.data, 2, 2, 0) == 0
    assert b"dimension out of range" in clib.proxtv_last_error()
    assert bool((out == 7.0).all())
    assert clib.proxtv_tv1_fibres_vjp_dev(y.data_ptr(), g.data_ptr(), out.data_ptr(), 0, 0, ns.ctypes.data, 2, 1, 0) == 1
    assert bool((out == 1.0).all())        # y is flat: one segment per fibre, the mean of ones
