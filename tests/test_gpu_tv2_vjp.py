"""The derivative of the TV-L2 fibre prox on the GPU: the multiplier output of proxtv_tv2_fibres_dev, proxtv_tv2_fibres_vjp_dev through
device.tv2_fibres_vjp, and the autograd wrapper.  The yardstick is the numpy model of tests/tv2_vjp_model.py (checked against central
differences of the CPU oracle in tests/test_tv2_vjp_host.py) applied to the DEVICE's y and mu, within
64 n 2^-52 cond(T + mu I) max|g|; the autograd tests difference the device function itself."""
import numpy as np
import pytest

import tv2_vjp_model as tm
import vjp_model as vm

pytestmark = pytest.mark.gpu

SHAPE = (150, 70, 5)
LAMS = (0.8, 40.0)


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


def dual_norms(x, dim):
    """||T^-1 D x|| of every fibre along `dim` (the oracle's branch: inside iff <= lambda), column-major order of the rest."""
    n = x.shape[dim]
    rest = np.delete(x.shape, dim)
    if n < 2:
        return np.zeros(int(np.prod(rest)))
    dx = np.diff(np.moveaxis(x, dim, -1), axis=-1)
    u = dx @ np.linalg.inv(tm.tmat(n)).T
    return np.linalg.norm(u, axis=-1).ravel(order="F")


@pytest.fixture(scope="module")
def array(dev, clib):
    """The (150, 70, 5) array, its cotangent and, per (dim, lambda), the device's forward with mu -- computed once, never modified."""
    rng = np.random.default_rng(2027)
    x, c = rng.standard_normal(SHAPE), rng.standard_normal(SHAPE)
    xd = dev.up(x)
    fwd = {}
    for dim in range(3):
        for lam in LAMS:
            y, mu = dev.device.tv2_fibres(xd, lam, dim, return_mu=True)
            fwd[dim, lam] = (y, mu, dev.down(y), dev.down(mu).ravel(order="F"))
    return x, c, xd, fwd


# ---- 4. mu and the forward -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [0, 1, 2])
def test_mu_and_the_forward(dev, clib, array, dim):
    torch = dev.torch
    x, c, xd, fwd = array
    ns = np.array(SHAPE, dtype=np.int32)
    both = []
    for lam in LAMS:
        y, mu, yh, muh = fwd[dim, lam]
        assert tuple(mu.shape) == tuple(np.delete(SHAPE, dim)) and mu.dtype == torch.float64
        # the same bits as the p = 2 arm of proxtv_tvp_fibres_dev
        yp = dev.device.colmajor_empty(SHAPE)
        torch.cuda.synchronize()
        assert clib.proxtv_tvp_fibres_dev(xd.data_ptr(), yp.data_ptr(), ns.ctypes.data, 3, dim, lam, 2.0, 0) == 1
        assert torch.equal(y, yp), (dim, lam)
        assert torch.equal(dev.device.tv2_fibres(xd, lam, dim), y)        # (mu == NULL: the same bits again)
        un = dual_norms(x, dim)
        assert np.min(np.abs(un - lam)) > 1e-9 * lam                       # (no fibre sits on the kink: the branch is decided)
        inside = un <= lam
        assert np.all(muh[inside] == 0.0), (dim, lam)
        assert np.all(muh[~inside] > 0.0), (dim, lam)
        want = np.linalg.norm(np.diff(np.moveaxis(yh, dim, -1), axis=-1), axis=-1).ravel(order="F") / lam
        rel = np.max(np.abs(muh[~inside] - want[~inside]) / want[~inside]) if np.any(~inside) else 0.0
        print(f"dim {dim} lambda {lam}: {int(inside.sum())} inside, {int((~inside).sum())} active, |mu - ||Dy||/lam| rel {rel:.2e}")
        assert rel <= 1e-9, (dim, lam)
        both.append(bool(inside.any() and (~inside).any()))
    # both branches occur in ONE array for at least one of the penalties, and both occur over the two
    assert any(both), dim


def test_both_branches_in_one_array(array):
    """lambda = 40 along the 150-sample dimension and lambda = 0.8 along the 5-sample one mix inside and active fibres."""
    x, c, xd, fwd = array
    for dim, lam in ((0, 40.0), (2, 0.8)):
        mu = fwd[dim, lam][3]
        assert np.any(mu == 0.0) and np.any(mu > 0.0), (dim, lam)


# ---- 5. the device against the model -------------------------------------------------------------------------------------------------------
def check_against_model(dev, y, mu, g, lam, dim, what):
    """gx and per-fibre glam of one device call against the model on the device's own y and mu; returns the device results."""
    gx, glam = dev.device.tv2_fibres_vjp(y, mu, dev.up(g), lam, dim, need_glam=True)
    yh, muh = dev.down(y), dev.down(mu).ravel(order="F")
    n = yh.shape[dim]
    want_gx, want_glam = tm.vjp_nd(yh, muh, g, lam, dim)
    gmax = np.max(np.abs(np.moveaxis(g, dim, -1)), axis=-1).ravel(order="F")
    bound = 64.0 * n * 2.0 ** -52 * tm.cond(n, muh) * gmax                         # per fibre (tm.bar)
    ex = np.max(np.abs(np.moveaxis(dev.down(gx) - want_gx, dim, -1)), axis=-1).ravel(order="F")
    el = np.abs(dev.down(glam).ravel(order="F") - want_glam)
    print(f"{what}: worst |gx - model| / bar {np.max(ex / bound):.2e}, worst |glam - model| / bar {np.max(el / bound):.2e}")
    assert np.all(ex <= bound), what
    assert np.all(el <= bound), what
    assert tuple(glam.shape) == tuple(mu.shape)
    return gx, glam


@pytest.mark.parametrize("dim", [0, 1, 2])
def test_array_against_the_model_in_place_and_reproducible(dev, array, dim):
    torch = dev.torch
    x, c, xd, fwd = array
    for lam in LAMS:
        y, mu = fwd[dim, lam][:2]
        gx, glam = check_against_model(dev, y, mu, c, lam, dim, f"shape {SHAPE} dim {dim} lambda {lam}")
        muh = fwd[dim, lam][3]
        assert np.all(dev.down(glam).ravel(order="F")[muh == 0.0] == 0.0)
        # twice: the same bits
        gx2, glam2 = dev.device.tv2_fibres_vjp(y, mu, dev.up(c), lam, dim, need_glam=True)
        assert torch.equal(gx, gx2) and torch.equal(glam, glam2)
        # in place: gx is g
        g = dev.up(c)
        gx3, glam3 = dev.device.tv2_fibres_vjp(y, mu, g, lam, dim, need_glam=True, out=g)
        assert gx3 is g and torch.equal(gx3, gx) and torch.equal(glam3, glam)
        # without glam; a cotangent in another layout is copied
        assert torch.equal(dev.device.tv2_fibres_vjp(y, mu, torch.from_numpy(np.ascontiguousarray(c)).cuda(), lam, dim), gx)


@pytest.mark.parametrize("shape,dim", [((1, 9), 0), ((2, 9), 0), ((3, 9), 0), ((9, 1), 1), ((9, 2), 1), ((9, 3), 1)])
def test_fibres_of_length_1_2_3(dev, shape, dim):
    rng = np.random.default_rng(90 + shape[dim])
    x, c = rng.standard_normal(shape), rng.standard_normal(shape)
    for lam in (0.8, 0.0):
        y, mu = dev.device.tv2_fibres(dev.up(x), lam, dim, return_mu=True)
        gx, glam = check_against_model(dev, y, mu, c, lam, dim, f"shape {shape} dim {dim} lambda {lam}")
        if shape[dim] == 1 or lam == 0.0:
            assert np.array_equal(dev.down(gx), c) and not dev.down(glam).any() and not dev.down(mu).any()


# ---- 6. the long route ---------------------------------------------------------------------------------------------------------------------
def test_long_fibre(dev, clib):
    torch = dev.torch
    n, lam = 20000, 0.5
    rng = np.random.default_rng(6)
    x, c = rng.standard_normal(n), rng.standard_normal(n)
    before = clib.proxtv_debug_counter(b"tv2_long_fibres")
    y, mu = dev.device.tv2_fibres(dev.up(x), lam, 0, return_mu=True)
    assert clib.proxtv_debug_counter(b"tv2_long_fibres") == before + 1          # the forward took tv2_long_*
    yh, muh = dev.down(y), float(mu)
    assert mu.shape == () and muh > 0.0
    assert abs(muh - np.linalg.norm(np.diff(yh)) / lam) <= 1e-9 * muh
    assert torch.equal(y, dev.device.tv2_fibres(dev.up(x), lam, 0))
    gx, glam = dev.device.tv2_fibres_vjp(y, mu, dev.up(c), lam, 0, need_glam=True)
    want_gx, want_glam = tm.vjp_1d(yh, muh, c, lam, banded=True)
    bound = tm.bar(n, muh, c)
    ex, el = float(np.max(np.abs(dev.down(gx) - want_gx))), abs(float(glam) - want_glam)
    print(f"long fibre: mu {muh:.3e}, |gx - model| {ex:.2e}, |glam - model| {el:.2e}, bar {bound:.2e}")
    assert ex <= bound and el <= bound
    gx2, glam2 = dev.device.tv2_fibres_vjp(y, mu, dev.up(c), lam, 0, need_glam=True)
    assert torch.equal(gx, gx2) and torch.equal(glam, glam2)
    g = dev.up(c)
    assert torch.equal(dev.device.tv2_fibres_vjp(y, mu, g, lam, 0, out=g), gx)
    # a penalty that flattens the fibre: inside, the mean of g on every sample
    y, mu = dev.device.tv2_fibres(dev.up(x), 1e9, 0, return_mu=True)
    assert float(mu) == 0.0
    gx, glam = dev.device.tv2_fibres_vjp(y, mu, dev.up(c), 1e9, 0, need_glam=True)
    gxh = dev.down(gx)
    assert float(glam) == 0.0 and np.all(gxh == gxh[0]) and abs(gxh[0] - c.mean()) <= vm.rounding_bound(n, c)


def test_many_long_fibres_stay_lane_per_fibre(dev, clib):
    n, count, lam = 16384, 48, 0.5
    rng = np.random.default_rng(7)
    x, c = rng.standard_normal((n, count)), rng.standard_normal((n, count))
    before = clib.proxtv_debug_counter(b"tv2_long_fibres")
    y, mu = dev.device.tv2_fibres(dev.up(x), lam, 0, return_mu=True)
    assert clib.proxtv_debug_counter(b"tv2_long_fibres") == before
    gx, glam = dev.device.tv2_fibres_vjp(y, mu, dev.up(c), lam, 0, need_glam=True)
    yh, muh, gxh, glamh = dev.down(y), dev.down(mu), dev.down(gx), dev.down(glam)
    for j in (0, 23, 47):
        assert muh[j] > 0.0
        want_gx, want_glam = tm.vjp_1d(yh[:, j], muh[j], c[:, j], lam, banded=True)
        bound = tm.bar(n, muh[j], c[:, j])
        ex, el = float(np.max(np.abs(gxh[:, j] - want_gx))), abs(glamh[j] - want_glam)
        print(f"fibre {j} of {count} x {n}: mu {muh[j]:.3e}, |gx - model| {ex:.2e}, |glam - model| {el:.2e}, bar {bound:.2e}")
        assert ex <= bound and el <= bound


# ---- 7. autograd ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [0, 1])
def test_autograd_against_central_differences(dev, dim):
    from proxtv_amd import autograd
    torch = dev.torch
    rng = np.random.default_rng(70)
    shape = (12, 10)
    x, c = rng.standard_normal(shape), rng.standard_normal(shape)
    lam, h = 0.8, vm.FD_H
    cd = dev.up(c)
    un = dual_norms(x, dim)
    assert np.all(np.abs(un - lam) >= tm.KINK_CLEAR * lam)       # (a property of the inputs: no fibre near the kink)

    def loss(xa, w):
        return float((cd * dev.device.tv2_fibres(dev.up(xa), w, dim)).sum())

    xt = dev.up(x).requires_grad_(True)
    wt = torch.tensor(lam, dtype=torch.float64, requires_grad=True)
    y = autograd.tv2_fibres(xt, wt, dim)
    assert torch.equal(y.detach(), dev.device.tv2_fibres(dev.up(x), lam, dim))
    gxt, gwt = torch.autograd.grad((cd * y).sum(), (xt, wt))
    assert gxt.dtype == torch.float64 and gxt.device == xt.device and dev.device._is_colmajor(gxt)
    assert gwt.device == wt.device and gwt.shape == ()
    ex = float(np.max(np.abs(dev.down(gxt) - vm.central_x(lambda a: loss(a, lam), np.ascontiguousarray(x).copy()))))
    ew = abs(float(gwt) - (loss(x, lam + h) - loss(x, lam - h)) / (2 * h))
    print(f"dim {dim}: |grad x - fd| {ex:.2e}, |grad w - fd| {ew:.2e}")
    assert ex <= vm.FD_TOL and ew <= vm.FD_TOL
    # only x asks: no glam is computed; nothing asks: the plain device call
    xt2 = dev.up(x).requires_grad_(True)
    (cd * autograd.tv2_fibres(xt2, lam, dim)).sum().backward()
    assert torch.equal(xt2.grad, gxt)
    assert autograd.tv2_fibres(dev.up(x), lam, dim).grad_fn is None


# ---- 8. composition: PD2 with a TV-L1 term along dimension 0 and a TV-L2 term along dimension 1 -----------------------------------------------
def test_composed_pd2_forward_and_backward(dev, ptv):
    from proxtv_amd import autograd
    torch = dev.torch
    rng = np.random.default_rng(80)
    X, c = rng.standard_normal((12, 10)), rng.standard_normal((12, 10))
    lams, iters = (0.6, 0.4), 5
    cd = dev.up(c)

    def pd2(xin, check=False):
        """x = y, p = q = 0; z = prox_0(x + p), p += x - z, x' = prox_1(z + q), q += z - x' (solvers.hip: pd2)."""
        x, p, q = xin, torch.zeros_like(xin), torch.zeros_like(xin)
        for _ in range(iters):
            z = autograd.tv1_fibres(x + p, lams[0], 0)
            p = p + x - z
            xn = autograd.tv2_fibres(z + q, lams[1], 1)
            if check:   # the operands keep clear of the kinks of both proxes, at every iteration
                vm.assert_unambiguous(dev.down(z.detach()), axis=0)
                un = dual_norms(dev.down((z + q).detach()), 1)
                assert not np.any(tm.near_kink(un, lams[1])), un
            q = q + z - xn
            x = xn
        return x

    xt = dev.up(X).requires_grad_(True)
    out = pd2(xt, check=True)
    want = ptv.tvgen(X, [0.6, 0.4], [1, 2], [1, 2], max_iters=5)
    ef = float(np.max(np.abs(dev.down(out.detach()) - want)))
    print(f"composed PD2 forward vs tvgen: {ef:.2e}")
    assert ef <= 1e-9
    (gx,) = torch.autograd.grad((cd * out).sum(), xt)
    gxh = dev.down(gx)
    pix = [(int(i), int(j)) for i, j in zip(rng.integers(0, 12, 8), rng.integers(0, 10, 8))]
    worst = 0.0
    with torch.no_grad():
        for i, j in pix:
            vals = []
            for s in (1.0, -1.0):
                Xp = X.copy()
                Xp[i, j] += s * vm.FD_H
                vals.append(float((cd * pd2(dev.up(Xp))).sum()))
            worst = max(worst, abs((vals[0] - vals[1]) / (2 * vm.FD_H) - gxh[i, j]))
    print(f"composed PD2 backward vs central differences at {len(pix)} pixels: {worst:.2e}")
    assert worst <= 1e-7


# ---- 9. argument checks --------------------------------------------------------------------------------------------------------------------
def test_argument_checks(dev, clib):
    torch = dev.torch
    rng = np.random.default_rng(9)
    x = dev.up(rng.standard_normal((6, 4)))
    y, mu = dev.device.tv2_fibres(x, 0.5, 0, return_mu=True)
    g = dev.up(np.ones((6, 4)))
    ns = np.array([6, 4], dtype=np.int32)
    out = torch.full_like(g, 7.0)
    glam = torch.full_like(mu, 7.0)
    y0, mu0 = y.clone(), mu.clone()
    torch.cuda.synchronize()     # (the C calls below run on the library's own stream)
    vjp = clib.proxtv_tv2_fibres_vjp_dev
    P = lambda t: t.data_ptr()   # noqa: E731
    untouched = lambda: bool((out == 7.0).all()) and bool((glam == 7.0).all()) and torch.equal(y, y0) and torch.equal(mu, mu0)   # noqa: E731
    # a dimension out of range
    for dim in (-1, 2):
        assert vjp(P(y), P(mu), P(g), P(out), P(glam), ns.ctypes.data, 2, dim, 0.5, 0) == 0
        assert b"dimension out of range" in clib.proxtv_last_error() and untouched()
    # missing pointers
    for args in ((0, P(mu), P(g), P(out)), (P(y), 0, P(g), P(out)), (P(y), P(mu), 0, P(out)), (P(y), P(mu), P(g), 0)):
        assert vjp(*args, P(glam), ns.ctypes.data, 2, 0, 0.5, 0) == 0
        assert b"required" in clib.proxtv_last_error() and untouched()
    # overlaps: gx on y, gx on g but shifted, glam on mu, glam inside gx
    for args in ((P(y), P(mu), P(g), P(y), P(glam)), (P(y), P(mu), P(g), P(g) + 8, P(glam)), (P(y), P(mu), P(g), P(out), P(mu)),
                 (P(y), P(mu), P(g), P(out), P(out) + 16)):
        assert vjp(*args, ns.ctypes.data, 2, 0, 0.5, 0) == 0
        assert b"overlaps" in clib.proxtv_last_error() and untouched() and bool((g == 1.0).all())
    # an empty array
    empty = np.array([0, 4], dtype=np.int32)
    assert vjp(0, 0, 0, 0, 0, empty.ctypes.data, 2, 0, 0.5, 0) == 1 and untouched()
    assert clib.proxtv_tv2_fibres_dev(0, 0, 0, empty.ctypes.data, 2, 1, 0.5, 0) == 1
    # the forward: a dimension out of range, mu on the output
    assert clib.proxtv_tv2_fibres_dev(P(x), P(out), P(glam), ns.ctypes.data, 2, 2, 0.5, 0) == 0 and untouched()
    assert clib.proxtv_tv2_fibres_dev(P(x), P(out), P(out), ns.ctypes.data, 2, 0, 0.5, 0) == 0
    assert b"overlaps" in clib.proxtv_last_error() and untouched()
    # and the call that is fine: gx == g exactly
    assert vjp(P(y), P(mu), P(g), P(g), P(glam), ns.ctypes.data, 2, 0, 0.5, 0) == 1
    want, want_glam = dev.device.tv2_fibres_vjp(y, mu, dev.up(np.ones((6, 4))), 0.5, 0, need_glam=True)
    assert torch.equal(g, want) and torch.equal(glam, want_glam)
    # the Python layer
    for dim in (-1, 2):
        with pytest.raises(ValueError):
            dev.device.tv2_fibres(x, 0.5, dim)
        with pytest.raises(ValueError):
            dev.device.tv2_fibres_vjp(y, mu, g, 0.5, dim)
    with pytest.raises(ValueError):
        dev.device.tv2_fibres_vjp(y, mu[:3], g, 0.5, 0)
    with pytest.raises(ValueError):
        dev.device.tv2_fibres_vjp(y, mu, g.float(), 0.5, 0)
