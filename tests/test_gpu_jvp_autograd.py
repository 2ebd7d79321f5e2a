"""torch's forward-mode AD through proxtv_amd.autograd: under ``torch.autograd.forward_ad.dual_level()`` the tangents out of tv1_fibres,
tv1_2d, tv1w_2d and tv1_2d_batch are the device.*_jvp calls bit for bit, the primals are the non-dual calls bit for bit, and plain
tensors get what they always got."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(ptv):
    import torch
    import torch.autograd.forward_ad as fw
    from proxtv_amd import autograd, device

    class Env:
        pass

    e = Env()
    e.torch, e.fw, e.autograd, e.device = torch, fw, autograd, device
    rng = np.random.default_rng(77)
    e.up = lambda a: device.to_colmajor(torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda())
    e.x, e.dx = e.up(rng.standard_normal((33, 65))), e.up(rng.standard_normal((33, 65)))
    e.wc, e.wr = e.up(rng.uniform(0.05, 0.5, (32, 65))), e.up(rng.uniform(0.05, 0.5, (33, 64)))
    e.dwc, e.dwr = e.up(rng.uniform(-1, 1, (32, 65))), e.up(rng.uniform(-1, 1, (33, 64)))
    e.xs, e.dxs = e.up(rng.standard_normal((20, 17, 3))), e.up(rng.standard_normal((20, 17, 3)))
    e.scalar = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
    return e


@pytest.mark.parametrize("dim", (0, 1))
def test_tv1_fibres(env, dim):
    torch, fw, autograd, device = env.torch, env.fw, env.autograd, env.device
    y = device.tv1_fibres(env.x, 0.5, dim)
    w, dw = (env.wc, env.dwc) if dim == 0 else (env.wr, env.dwr)
    yw = device.tv1_fibres(env.x, 0.0, dim, w)
    with fw.dual_level():
        out = fw.unpack_dual(autograd.tv1_fibres(fw.make_dual(env.x, env.dx), 0.5, dim))
        assert torch.equal(out.primal, y) and torch.equal(out.tangent, device.tv1_fibres_jvp(y, env.dx, dim))
        lam = fw.make_dual(env.scalar(0.5), env.scalar(2.0))
        out = fw.unpack_dual(autograd.tv1_fibres(fw.make_dual(env.x, env.dx), lam, dim))
        assert torch.equal(out.primal, y) and torch.equal(out.tangent, device.tv1_fibres_jvp(y, env.dx, dim, dw=2.0))
        out = fw.unpack_dual(autograd.tv1_fibres(env.x, lam, dim))          # the penalty alone
        assert torch.equal(out.primal, y) and torch.equal(out.tangent, device.tv1_fibres_jvp(y, None, dim, dw=2.0))
        out = fw.unpack_dual(autograd.tv1_fibres(fw.make_dual(env.x, env.dx), 0.0, dim, weights=fw.make_dual(w, dw)))
        assert torch.equal(out.primal, yw) and torch.equal(out.tangent, device.tv1_fibres_jvp(yw, env.dx, dim, dweights=dw))
        out = fw.unpack_dual(autograd.tv1_fibres(fw.make_dual(env.x, env.dx), 0.5, dim, tape="steps"))
        assert torch.equal(out.tangent, device.tv1_fibres_jvp(y, env.dx, dim))


def test_tv1_2d_with_a_dual_image_and_a_dual_penalty(env):
    torch, fw, autograd, device = env.torch, env.fw, env.autograd, env.device
    y = device.tv1_2d(env.x, 0.1, 35)[0]
    y2 = device.tv1_2d(env.x, 0.1, 35, w_row=0.07)[0]
    with fw.dual_level():
        lam = fw.make_dual(env.scalar(0.1), env.scalar(1.0))
        out = fw.unpack_dual(autograd.tv1_2d(fw.make_dual(env.x, env.dx), 0.1, 35))
        assert torch.equal(out.primal, y) and torch.equal(out.tangent, device.dr2_jvp(env.x, env.dx, 0.1, max_iters=35)[0])
        out = fw.unpack_dual(autograd.tv1_2d(env.x, lam, 35))                # one tensor for both directions: d lambda on both
        assert torch.equal(out.primal, y)
        assert torch.equal(out.tangent, device.dr2_jvp(env.x, None, 0.1, max_iters=35, dw_col=1.0, dw_row=1.0)[0])
        out = fw.unpack_dual(autograd.tv1_2d(fw.make_dual(env.x, env.dx), lam, 35, w_row=0.07))
        assert torch.equal(out.primal, y2)
        assert torch.equal(out.tangent, device.dr2_jvp(env.x, env.dx, 0.1, 0.07, max_iters=35, dw_col=1.0)[0])


def test_tv1w_2d_with_dual_maps(env):
    torch, fw, autograd, device = env.torch, env.fw, env.autograd, env.device
    y = device.tv1w_2d(env.x, env.wc, env.wr, 35)[0]
    with fw.dual_level():
        out = fw.unpack_dual(autograd.tv1w_2d(fw.make_dual(env.x, env.dx), fw.make_dual(env.wc, env.dwc), fw.make_dual(env.wr, env.dwr), 35))
        want = device.dr2_jvp(env.x, env.dx, 0.0, max_iters=35, weights_col=env.wc, weights_row=env.wr, dweights_col=env.dwc,
                              dweights_row=env.dwr)[0]
        assert torch.equal(out.primal, y) and torch.equal(out.tangent, want)
        out = fw.unpack_dual(autograd.tv1w_2d(env.x, fw.make_dual(env.wc, env.dwc), env.wr, 35))      # one map alone
        want = device.dr2_jvp(env.x, None, 0.0, max_iters=35, weights_col=env.wc, weights_row=env.wr, dweights_col=env.dwc)[0]
        assert torch.equal(out.primal, y) and torch.equal(out.tangent, want)


def test_tv1_2d_batch(env):
    torch, fw, autograd, device = env.torch, env.fw, env.autograd, env.device
    y = device.tv1_2d_batch(env.xs, 0.5, 35)[0]
    with fw.dual_level():
        lam = fw.make_dual(env.scalar(0.5), env.scalar(-1.5))
        out = fw.unpack_dual(autograd.tv1_2d_batch(fw.make_dual(env.xs, env.dxs), lam, 35))
        want = device.dr2_jvp(env.xs, env.dxs, 0.5, max_iters=35, dw_col=-1.5, dw_row=-1.5)[0]
        assert torch.equal(out.primal, y) and torch.equal(out.tangent, want)


def test_plain_tensors_get_what_they_always_got(env):
    torch, fw, autograd, device = env.torch, env.fw, env.autograd, env.device
    want = (device.tv1_fibres(env.x, 0.5, 0), device.tv1_2d(env.x, 0.1, 35)[0], device.tv1w_2d(env.x, env.wc, env.wr, 35)[0],
            device.tv1_2d_batch(env.xs, 0.5, 35)[0])
    for inside in (False, True):
        with fw.dual_level() if inside else torch.no_grad():
            got = (autograd.tv1_fibres(env.x, 0.5, 0), autograd.tv1_2d(env.x, 0.1, 35), autograd.tv1w_2d(env.x, env.wc, env.wr, 35),
                   autograd.tv1_2d_batch(env.xs, env.scalar(0.5), 35))
            for g, w in zip(got, want):
                assert torch.equal(g, w) and g.grad_fn is None and fw.unpack_dual(g).tangent is None
    # reverse mode is what it was: a gradient through the Function whose signature grew
    x = env.x.clone().requires_grad_(True)
    lam = env.scalar(0.1).requires_grad_(True)
    autograd.tv1_2d(x, lam, 35).sum().backward()
    gx, _, _, glam, _ = device.dr2_vjp(env.x, torch.ones_like(env.x), 0.1, max_iters=35, need_gw="sums")
    assert torch.equal(x.grad, gx) and float(lam.grad) == float(glam.sum())
    x = env.x.clone().requires_grad_(True)
    autograd.tv1_fibres(x, 0.5, 1).sum().backward()
    assert torch.equal(x.grad, device.tv1_fibres_vjp(device.tv1_fibres(env.x, 0.5, 1), torch.ones_like(env.x), 1)[0])
