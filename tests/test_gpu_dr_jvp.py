"""The forward-mode derivative of the 2-D Douglas-Rachford TV-L1 solves on the GPU: proxtv_DR2_TV_jvp_dev through device.dr2_jvp.
Yardsticks: the numpy model of tests/jvp_model.py (checked against central differences in tests/test_jvp_model.py), central differences
of the fused device solves themselves, and the existing device.dr2_vjp by the adjoint identity.  Tolerance of the model comparison:
64 max(M, N) 2^-52 times the sum over all sweeps of the 2-norm of the tangent entering that sweep, the norms reported by the model (6d's
argument with the tangents' own norms).  Inputs: unit Gaussian noise, lambda in {0.1, 0.5}, per-edge weights U(0.05, 0.5)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import dr_vjp_model as dm
import jvp_model as jm
import vjp_model as vm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# (seed, shape, lambda, weighted): uniform, weighted, and (B = 3) a batch; every one with max_iters 1 and 35
MODEL_CASES = ((41, (130, 70), 0.1, False), (42, (17, 1041), 0.5, False), (43, (1, 40), 0.5, False), (44, (40, 1), 0.1, False),
               (45, (33, 65), 0.0, True), (46, (20, 17, 3), 0.5, False))


@pytest.fixture(scope="module")
def dev(ptv):
    import torch
    from proxtv_amd import device

    class Dev:
        pass

    d = Dev()
    d.torch, d.device = torch, device
    d.up = lambda a: None if a is None else device.to_colmajor(torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda())
    d.down = lambda t: t.cpu().numpy()
    return d


def unit(a):
    m = float(np.max(np.abs(a))) if a.size else 0.0
    return a / m if m > 0 else a


@functools.lru_cache(maxsize=None)
def case(seed, shape, lam, weighted, maxit):
    """One case, once: inputs, tangents (largest entry 1), the model's tape per image.  Nobody writes into them."""
    from oracle import cpu
    rng = np.random.default_rng(seed)
    s1, s2 = jm.edge_shapes(shape)
    U, dU, g = rng.standard_normal(shape), unit(rng.standard_normal(shape)), rng.standard_normal(shape)
    W1m = rng.uniform(0.05, 0.5, s1) if weighted else None
    W2m = rng.uniform(0.05, 0.5, s2) if weighted else None
    dW1m, dW2m = unit(rng.uniform(-1.0, 1.0, s1)), unit(rng.uniform(-1.0, 1.0, s2))
    W1, W2 = (0.0, 0.0) if weighted else (lam, dm.ROW_RATIO * lam if len(shape) == 2 else lam)
    tapes = []
    for b in range(shape[2] if len(shape) == 3 else 1):
        pick = (lambda a: a) if len(shape) == 2 else (lambda a, b=b: None if a is None else a[:, :, b])
        out, tape = dm.forward(cpu.oracle(), pick(U), W1, W2, maxit, pick(W1m), pick(W2m))
        dm.assert_tape_unambiguous(tape)
        tapes.append(tape)
    for a in (U, dU, g, dW1m, dW2m):
        a.setflags(write=False)
    return dict(U=U, dU=dU, g=g, W1=W1, W2=W2, W1m=W1m, W2m=W2m, dW1m=dW1m, dW2m=dW2m, tapes=tapes, maxit=maxit, shape=shape)


def model_jvp(c, dU, dW1, dW2):
    """(ds, bound) of the model, image by image."""
    shape = c["shape"]
    ds, bound = np.empty(shape), 0.0
    for b, tape in enumerate(c["tapes"]):
        pick = (lambda a: a) if len(shape) == 2 else (lambda a, b=b: a[:, :, b])
        d, entering = jm.dr_jvp(tape, pick(dU), pick(dW1), pick(dW2))
        if len(shape) == 2:
            ds = d
        else:
            ds[:, :, b] = d
        bound = max(bound, 64.0 * max(shape[0], shape[1]) * 2.0 ** -52 * entering)
    return ds, bound


def call(dev, c, dU=None, dW1m=None, dW2m=None, dw_col=0.0, dw_row=0.0, **kw):
    return dev.device.dr2_jvp(dev.up(c["U"]), dev.up(dU), c["W1"], c["W2"], c["maxit"], weights_col=dev.up(c["W1m"]),
                              weights_row=dev.up(c["W2m"]), dw_col=dw_col, dw_row=dw_row, dweights_col=dev.up(dW1m),
                              dweights_row=dev.up(dW2m), **kw)


def dot(a, b):
    return float(np.sum(np.asarray(a, dtype=np.longdouble) * np.asarray(b, dtype=np.longdouble)))


# ---- 1. against the numpy model --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maxit", (1, 35))
@pytest.mark.parametrize("seed,shape,lam,weighted", MODEL_CASES)
def test_against_the_model(dev, seed, shape, lam, weighted, maxit):
    c = case(seed, shape, lam, weighted, maxit)
    s1, s2 = jm.edge_shapes(shape)
    z, z1, z2 = np.zeros(shape), np.zeros(s1), np.zeros(s2)
    worst = 0.0
    for what, kw, model_args in (("dU", dict(dU=c["dU"]), (c["dU"], z1, z2)),
                                 ("uniform", dict(dw_col=1.0, dw_row=-0.5), (z, z1 + 1.0, z2 - 0.5)),
                                 ("maps", dict(dW1m=c["dW1m"], dW2m=c["dW2m"]), (z, c["dW1m"], c["dW2m"])),
                                 ("all", dict(dU=c["dU"], dW1m=c["dW1m"], dW2m=c["dW2m"], dw_col=0.25, dw_row=0.5),
                                  (c["dU"], c["dW1m"] + 0.25, c["dW2m"] + 0.5))):
        want, bound = model_jvp(c, *model_args)
        dy, _ = call(dev, c, **kw)
        err = float(np.max(np.abs(dev.down(dy) - want)))
        worst = max(worst, err / bound)
        print(f"seed {seed} {shape} maxit {maxit} weighted {weighted} {what}: |ds - model| {err:.2e} (bar {bound:.2e}, ratio {err / bound:.4f})")
        assert err <= bound, (what, err, bound)
    print(f"seed {seed} {shape} maxit {maxit}: worst ratio {worst:.4f}")


# ---- 2. against central differences of the fused solves --------------------------------------------------------------------------------
def test_against_central_differences_of_the_fused_solves(dev):
    """130 x 70, h = 1e-5, bar 1e-8: in dx, in d lambda_col, in d lambda_row (device.tv1_2d) and in one per-edge map (device.tv1w_2d).
    The two displaced solves must share the segmentation of all 72 sweep outputs, and a central difference that straddles a kink -- a
    jump closing, or a segment splitting where its dual reaches the penalty, which no look at the jumps of the undisplaced solve shows --
    is off by a fraction of the change in slope.  At this size most seeds have such a kink within h of lambda: on the numpy model
    (CPU oracle, the same arithmetic as the fused solve up to rounding) the uniform directions straddle one for seeds 41-54 and 56-59 and
    are clean for 55 and 60; the per-edge map, which displaces 9030 penalties at once, is first clean at seed 89 of 41-89.  Those seeds
    were picked for that reason; the bar is untouched."""
    h, bar, device = vm.FD_H, vm.FD_TOL, dev.device
    c = case(55, (130, 70), 0.1, False, 35)
    U = c["U"]

    def fused(u, w1, w2):
        return dev.down(device.tv1_2d(dev.up(u), w1, 35, w_row=w2)[0])

    for what, kw, (du, d1, d2) in (("dx", dict(dU=c["dU"]), (c["dU"], 0.0, 0.0)), ("dlam_col", dict(dw_col=1.0), (0.0, 1.0, 0.0)),
                                   ("dlam_row", dict(dw_row=1.0), (0.0, 0.0, 1.0))):
        fd = (fused(U + h * du, c["W1"] + h * d1, c["W2"] + h * d2) - fused(U - h * du, c["W1"] - h * d1, c["W2"] - h * d2)) / (2 * h)
        err = float(np.max(np.abs(dev.down(call(dev, c, **kw)[0]) - fd)))
        print(f"(130, 70) {what}: |ds - fd| {err:.2e} (bar {bar:.0e})")
        assert err <= bar, what
    c = case(89, (130, 70), 0.0, True, 35)

    def fusedw(w1):
        return dev.down(device.tv1w_2d(dev.up(c["U"]), dev.up(w1), dev.up(c["W2m"]), 35)[0])

    fd = (fusedw(c["W1m"] + h * c["dW1m"]) - fusedw(c["W1m"] - h * c["dW1m"])) / (2 * h)
    err = float(np.max(np.abs(dev.down(call(dev, c, dW1m=c["dW1m"])[0]) - fd)))
    print(f"(130, 70) per-edge column map: |ds - fd| {err:.2e} (bar {bar:.0e})")
    assert err <= bar


# ---- 3. against dr2_vjp by the adjoint identity -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,shape,lam,weighted", MODEL_CASES)
def test_adjoint_identity_against_dr2_vjp(dev, seed, shape, lam, weighted):
    """<g, ds> = <gU, dU> + <gW1, dW1> + <gW2, dW2>: each side within its own rounding bound per element (forward mode: test 1's; reverse
    mode: dr_vjp_model.sweep_scale, twice that for the penalties) times the 1-norm of the vector it meets; extended-precision sums."""
    c = case(seed, shape, lam, weighted, 35)
    dW1, dW2 = c["dW1m"] + 0.25, c["dW2m"] - 0.5
    ds = dev.down(call(dev, c, dU=c["dU"], dW1m=c["dW1m"], dW2m=c["dW2m"], dw_col=0.25, dw_row=-0.5)[0])
    gx, gwc, gwr, _, _ = dev.device.dr2_vjp(dev.up(c["U"]), dev.up(c["g"]), c["W1"], c["W2"], 35, weights_col=dev.up(c["W1m"]),
                                            weights_row=dev.up(c["W2m"]), need_gw=True)
    defect = abs(dot(c["g"], ds) - dot(dev.down(gx), c["dU"]) - dot(dev.down(gwc), dW1) - dot(dev.down(gwr), dW2))
    _, fwd_bound = model_jvp(c, c["dU"], dW1, dW2)
    rev = max(dm.sweep_scale(shape, 35, c["g"][..., b] if len(shape) == 3 else c["g"]) for b in range(shape[2] if len(shape) == 3 else 1))
    bound = fwd_bound * np.abs(c["g"]).sum() + rev * (np.abs(c["dU"]).sum() + 2 * np.abs(dW1).sum() + 2 * np.abs(dW2).sum())
    print(f"seed {seed} {shape} weighted {weighted}: adjoint defect {defect:.2e} (bar {bound:.2e}), <g, ds> = {dot(c['g'], ds):.6f}")
    assert defect <= bound


# ---- 4. bits ------------------------------------------------------------------------------------------------------------------------------
def test_bits(dev, clib):
    torch, device = dev.torch, dev.device
    c = case(41, (130, 70), 0.1, False, 35)
    kw = dict(dU=c["dU"], dW1m=c["dW1m"], dW2m=c["dW2m"], dw_col=0.25, dw_row=0.5)
    dy, y = call(dev, c, need_y=True, **kw)
    dy2, y2 = call(dev, c, need_y=True, **kw)
    assert torch.equal(dy, dy2) and torch.equal(y, y2)                                     # two calls, the same bits
    yv = device.dr2_vjp(dev.up(c["U"]), dev.up(c["g"]), c["W1"], c["W2"], 35, need_y=True)[4]
    assert torch.equal(y, yv)                                                              # the forward of dr2_vjp, bit for bit
    zero, _ = call(dev, c)
    assert torch.equal(zero, torch.zeros_like(zero))                                       # no tangent: exact zeros
    zero, _ = call(dev, c, dU=np.zeros((130, 70)), dW1m=np.zeros((129, 70)), dW2m=np.zeros((130, 69)))
    assert torch.equal(zero, torch.zeros_like(zero))
    try:                                                                                   # both routes of the three-array combination
        routes = []
        for route in (1, 2):
            clib.proxtv_set_option(b"dr_jvp_route", route)
            routes.append(call(dev, c, **kw)[0])
    finally:
        clib.proxtv_set_option(b"dr_jvp_route", 0)
    assert torch.equal(routes[0], routes[1]) and torch.equal(routes[0], dy)
    cw = case(45, (33, 65), 0.0, True, 35)
    for route in (1, 2):
        try:
            clib.proxtv_set_option(b"dr_jvp_route", route)
            got = call(dev, cw, dU=cw["dU"], dW1m=cw["dW1m"], dW2m=cw["dW2m"])[0]
        finally:
            clib.proxtv_set_option(b"dr_jvp_route", 0)
        assert torch.equal(got, call(dev, cw, dU=cw["dU"], dW1m=cw["dW1m"], dW2m=cw["dW2m"])[0])


def test_an_image_of_a_batch_has_the_bits_of_its_own_call(dev):
    torch, device = dev.torch, dev.device
    c = case(46, (20, 17, 3), 0.5, False, 35)
    dy, y = call(dev, c, dU=c["dU"], dW1m=c["dW1m"], dW2m=c["dW2m"], dw_col=0.25, need_y=True)
    for b in range(3):
        one, y1 = device.dr2_jvp(dev.up(c["U"][:, :, b]), dev.up(c["dU"][:, :, b]), c["W1"], c["W2"], 35, dw_col=0.25,
                                 dweights_col=dev.up(c["dW1m"][:, :, b]), dweights_row=dev.up(c["dW2m"][:, :, b]), need_y=True)
        assert torch.equal(dy[:, :, b], one) and torch.equal(y[:, :, b], y1), b


# ---- 5. constant scratch ------------------------------------------------------------------------------------------------------------------
def test_scratch_does_not_grow_with_the_iterations():
    """A child process with the scratch pool capped at 1 MiB: dr2_jvp of a 64 x 64 image goes through at 35 and at 2000 iterations, dr2_vjp
    is refused at 2000 under both tapes."""
    env = dict(os.environ, PROXTV_POOL_CAP_MB="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "dr_jvp_cap_child.py")], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "JVP_CAP_CHILD_OK" in r.stdout


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(dev, clib):
    torch, device = dev.torch, dev.device
    c = case(45, (33, 65), 0.0, True, 35)
    U, W1m, W2m, dU = dev.up(c["U"]), dev.up(c["W1m"]), dev.up(c["W2m"]), dev.up(c["dU"])
    with pytest.raises(ValueError, match="pairs"):
        device.dr2_jvp(U, dU, 0.1, weights_col=W1m)
    with pytest.raises(ValueError, match="dx: shape"):
        device.dr2_jvp(U, dev.up(np.zeros((33, 64))), 0.1)
    with pytest.raises(ValueError, match="dweights_row: shape"):
        device.dr2_jvp(U, dU, 0.1, dweights_row=dev.up(np.zeros((32, 65))))
    with pytest.raises(ValueError, match="float64"):
        device.dr2_jvp(U, dU.float(), 0.1)
    with pytest.raises(ValueError, match="column-major"):
        device.dr2_jvp(U.contiguous(), dU, 0.1)
    # straight through the C-ABI: exactly one weight map; ds overlapping an input; a missing ds -- each returns 0, names the reason and
    # leaves the outputs alone
    n = 33 * 65
    out = torch.full((2 * n,), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s, ds = out.data_ptr(), out.data_ptr() + 8 * n
    rc = clib.proxtv_DR2_TV_jvp_dev(33, 65, 1, U.data_ptr(), 0.1, 0.1, W1m.data_ptr(), 0, dU.data_ptr(), 0, 0, 0.0, 0.0, s, ds, 35, 0)
    assert rc == 0 and b"pairs" in clib.proxtv_last_error() and bool((out == 7.0).all())
    rc = clib.proxtv_DR2_TV_jvp_dev(33, 65, 1, U.data_ptr(), 0.1, 0.1, 0, 0, dU.data_ptr(), 0, 0, 0.0, 0.0, s, s + 8, 35, 0)
    assert rc == 0 and b"overlaps" in clib.proxtv_last_error() and bool((out == 7.0).all())
    rc = clib.proxtv_DR2_TV_jvp_dev(33, 65, 1, out.data_ptr(), 0.1, 0.1, 0, 0, 0, 0, 0, 1.0, 0.0, 0, ds - 8, 35, 0)
    assert rc == 0 and b"overlaps" in clib.proxtv_last_error() and bool((out == 7.0).all())
    rc = clib.proxtv_DR2_TV_jvp_dev(33, 65, 1, U.data_ptr(), 0.1, 0.1, 0, 0, dU.data_ptr(), 0, 0, 0.0, 0.0, s, 0, 35, 0)
    assert rc == 0 and b"required" in clib.proxtv_last_error() and bool((out == 7.0).all())
    assert clib.proxtv_DR2_TV_jvp_dev(0, 65, 1, 0, 0.1, 0.1, 0, 0, 0, 0, 0, 0.0, 0.0, 0, 0, 35, 0) == 1      # nothing to do
