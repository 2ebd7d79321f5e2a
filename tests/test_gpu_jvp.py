"""The forward-mode derivative of the TV-L1 fibre prox on the GPU: proxtv_tv1_fibres_jvp_dev through device.tv1_fibres_jvp.  Yardsticks:
the numpy model of tests/jvp_model.py (checked against central differences in tests/test_jvp_model.py) within the certifier's rounding
rule, 64 n 2^-52 max|v| (n the fibre length, v = dx + E from the model), and the existing device.tv1_fibres_vjp by the adjoint identity
<g, dy> = <gx, dx> + <gw, dr>, which needs no model.  Inputs: unit Gaussian noise, lambda in {0.1, 0.5}, per-edge weights U(0.05, 0.5)."""
import functools

import numpy as np
import pytest

import jvp_model as jm
import vjp_model as vm

pytestmark = pytest.mark.gpu

SHAPES = ((1, 5), (17, 3), (16, 64), (33, 65), (1041, 2), (2, 1041), (5, 7, 6))
CASES = [(shape, dim) for shape in SHAPES for dim in range(len(shape))]


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


def edge_shape(shape, dim):
    s = list(shape)
    s[dim] = max(s[dim] - 1, 0)
    return tuple(s)


@functools.lru_cache(maxsize=None)
def draw(shape, dim, weighted):
    rng = np.random.default_rng(1000 * len(shape) + 10 * int(np.prod(shape)) + dim + (500 if weighted else 0))
    lam = (0.1, 0.5)[(dim + len(shape)) % 2]
    x, dx, g = rng.standard_normal(shape), rng.standard_normal(shape), rng.standard_normal(shape)
    w = rng.uniform(0.05, 0.5, edge_shape(shape, dim)) if weighted else None
    dw = rng.uniform(-1.0, 1.0, edge_shape(shape, dim))
    for a in (x, dx, g, dw):
        a.setflags(write=False)
    return x, dx, g, lam, w, dw


def prox(dev, shape, dim, weighted):
    x, dx, g, lam, w, dw = draw(shape, dim, weighted)
    y = dev.device.tv1_fibres(dev.up(x), lam, dim, None if w is None else dev.up(w))
    d = np.abs(np.diff(dev.down(y), axis=dim))      # no jump within reach of the step rule (below 1e-12: rounding inside a segment)
    assert not np.any((d >= 1e-12) & (d <= 1e-6)), (shape, dim, weighted)
    return y


def dot(a, b):
    return float(np.sum(np.asarray(a, dtype=np.longdouble) * np.asarray(b, dtype=np.longdouble)))


@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("shape,dim", CASES)
def test_against_the_model(dev, shape, dim, weighted):
    x, dx, g, lam, w, dw = draw(shape, dim, weighted)
    y = prox(dev, shape, dim, weighted)
    yn, n = dev.down(y), shape[dim]
    ones = np.ones(edge_shape(shape, dim))
    for what, a, b, dlam in (("dx", dx, None, 0.0), ("uniform", None, None, 1.0), ("per edge", None, dw, 0.0), ("all", dx, dw, -0.4)):
        want, v = jm.jvp_nd(yn, np.zeros(shape) if a is None else a, (0.0 * ones if b is None else b) + dlam * ones, dim)
        bound = vm.rounding_bound(n, v) if v.size else 0.0
        dy = dev.device.tv1_fibres_jvp(y, None if a is None else dev.up(a), dim, dweights=None if b is None else dev.up(b), dw=dlam)
        err = float(np.max(np.abs(dev.down(dy) - want)))
        print(f"{shape} dim {dim} weighted {weighted} {what}: |dy - model| {err:.2e} (bar {bound:.2e})")
        assert err <= bound, (what, err, bound)
        assert dev.torch.equal(dy, dev.device.tv1_fibres_jvp(y, None if a is None else dev.up(a), dim, dweights=None if b is None else dev.up(b), dw=dlam))
        if a is not None:    # dy aliasing dx: the same bits
            buf = dev.up(a)
            assert dev.device.tv1_fibres_jvp(y, buf, dim, dweights=None if b is None else dev.up(b), dw=dlam, out=buf) is buf
            assert dev.torch.equal(buf, dy), what


@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("shape,dim", CASES)
def test_adjoint_identity_against_the_vjp(dev, shape, dim, weighted):
    """|<g, dy> - <gx, dx> - <gw, dr>| within the sum of both calls' rounding-rule bounds, each times the 1-norm of the vector it meets in
    the inner product (gw is a difference of two means: twice the bound).  The inner products are taken in extended precision, so the
    test adds no rounding of its own.  A wrong sign of E or an edge off by one breaks this by O(1)."""
    x, dx, g, lam, w, dw = draw(shape, dim, weighted)
    y = prox(dev, shape, dim, weighted)
    n = shape[dim]
    dr = dw + 0.3
    dy = dev.down(dev.device.tv1_fibres_jvp(y, dev.up(dx), dim, dweights=dev.up(dw), dw=0.3))
    gx, gw, _ = dev.device.tv1_fibres_vjp(y, dev.up(g), dim, need_gw=True)
    gx, gw = dev.down(gx), dev.down(gw)
    _, v = jm.jvp_nd(dev.down(y), dx, dr, dim)
    defect = abs(dot(g, dy) - dot(gx, dx) - dot(gw, dr))
    bound = vm.rounding_bound(n, v) * np.abs(g).sum() + vm.rounding_bound(n, g) * (np.abs(dx).sum() + 2 * np.abs(dr).sum())
    print(f"{shape} dim {dim} weighted {weighted}: adjoint defect {defect:.2e} (bar {bound:.2e}), <g, dy> = {dot(g, dy):.6f}")
    assert defect <= bound


def test_zero_tangents_give_exact_zeros_and_one_sample_fibres_copy(dev):
    torch = dev.torch
    y = prox(dev, (33, 65), 0, False)
    assert torch.equal(dev.device.tv1_fibres_jvp(y, None, 0), torch.zeros_like(y))
    assert torch.equal(dev.device.tv1_fibres_jvp(y, torch.zeros_like(y), 1, dweights=dev.up(np.zeros((33, 64))), dw=0.0), torch.zeros_like(y))
    x, dx, *_ = draw((1, 5), 0, False)
    one = dev.device.tv1_fibres_jvp(dev.up(x), dev.up(dx), 0, dw=2.0)          # ns[dim] == 1: no edges, dy = dx
    assert torch.equal(one, dev.up(dx))


def test_refusals_write_nothing(dev, clib):
    torch, device = dev.torch, dev.device
    y = prox(dev, (33, 65), 0, False)
    dx = torch.ones_like(y)
    with pytest.raises(ValueError, match="dx: shape"):
        device.tv1_fibres_jvp(y, dev.up(np.zeros((33, 64))), 0)
    with pytest.raises(ValueError, match="dweights: shape"):
        device.tv1_fibres_jvp(y, dx, 0, dweights=dev.up(np.zeros((33, 64))))
    with pytest.raises(ValueError, match="float64"):
        device.tv1_fibres_jvp(y, dx.float(), 0)
    with pytest.raises(ValueError, match="column-major"):
        device.tv1_fibres_jvp(y.contiguous(), dx, 0)
    with pytest.raises(ValueError, match="out of range"):
        device.tv1_fibres_jvp(y, dx, 2)
    # straight through the C-ABI: dy overlapping y, and dy overlapping dx without being dx
    ns = np.array([33, 65], dtype=np.int32)
    flat = torch.full((2 * 33 * 65,), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for args in ((flat.data_ptr(), dx.data_ptr(), 0, 0.0, flat.data_ptr() + 8), (y.data_ptr(), flat.data_ptr(), 0, 0.0, flat.data_ptr() + 8)):
        rc = clib.proxtv_tv1_fibres_jvp_dev(*args, ns.ctypes.data, 2, 0, 0)
        assert rc == 0 and b"overlaps" in clib.proxtv_last_error()
        assert bool((flat == 7.0).all())
    assert clib.proxtv_tv1_fibres_jvp_dev(y.data_ptr(), dx.data_ptr(), 0, 0.0, 0, ns.ctypes.data, 2, 0, 0) == 0
    assert b"required" in clib.proxtv_last_error()
    assert clib.proxtv_tv1_fibres_jvp_dev(y.data_ptr(), dx.data_ptr(), 0, 0.0, flat.data_ptr(), ns.ctypes.data, 2, 5, 0) == 0
    assert bool((flat == 7.0).all())
