"""The tape of step codes on the GPU: proxtv_tv1_fibres_steps_dev / proxtv_tv1_fibres_vjp_steps_dev against the derivative from y, and
the solver derivatives with tape = 1 against tape = 0.  The chunk kernels take nothing from y but the codes, so every comparison in
this file is torch.equal / array_equal: there is no tolerance."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# (1025,): 65 chunks, two trips of phase B's wave scan; (5, 18, 3) along 1: strided with more than one block
SHAPES = ((1,), (2,), (15,), (16,), (17,), (33,), (1025,), (17, 1), (16, 65), (33, 63), (65, 17), (5, 18, 3), (3, 4, 35))
LAMBDAS = (1e-3, 1.0, 1e3)      # all steps ; segments across chunk edges ; one segment across every chunk


@pytest.fixture(scope="module")
def dev(ptv):
    import torch
    from proxtv_amd import device

    class Dev:
        pass

    d = Dev()
    d.torch, d.device = torch, device
    d.up = lambda a: device.to_colmajor(torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda())
    return d


@functools.lru_cache(maxsize=None)
def noise(shape, seed=0):
    a = np.random.default_rng(seed + 97 * len(shape) + sum(shape)).standard_normal(shape)
    a.setflags(write=False)
    return a


def same(torch, a, b):
    if a is None or b is None:
        return a is None and b is None
    return torch.equal(a, b) if isinstance(a, torch.Tensor) else np.array_equal(a, b)


def popcount16(words):
    w = words.cpu().numpy().astype(np.uint32) & 0xffff
    return int(sum(bin(int(v)).count("1") for v in w.ravel()))


# ---- 1. fibre level ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_words_give_the_bits_of_y(dev, clib, shape):
    torch, device = dev.torch, dev.device
    x, g = dev.up(noise(shape)), dev.up(noise(shape, 1))
    ns = np.array(shape, dtype=np.int32)
    for dim in range(len(shape)):
        fibres = int(np.prod(shape)) // shape[dim]
        for lam in LAMBDAS:
            y = device.tv1_fibres(x, lam, dim)
            steps = device.tv1_fibres_steps(y, dim)
            assert steps.dtype == torch.int32 and steps.dim() == 1
            assert steps.numel() == clib.proxtv_tv1_steps_words(ns.ctypes.data, len(shape), dim) == fibres * ((shape[dim] + 15) // 16)
            assert torch.equal(steps, device.tv1_fibres_steps(y, dim))
            gx, gw, nseg = device.tv1_fibres_vjp(y, g, dim, need_gw=True, need_nseg=True)
            gx2, gw2, nseg2 = device.tv1_fibres_vjp_steps(steps, g, shape, dim, need_gw=True, need_nseg=True)
            assert torch.equal(gx2, gx) and torch.equal(gw2, gw) and torch.equal(nseg2, nseg), (dim, lam)
            # the format: steps of a fibre = its segments less one; an up bit only on a step
            w = steps.cpu().numpy().astype(np.uint32)
            assert popcount16(steps) == int(nseg.sum()) - fibres, (dim, lam)
            assert not np.any((w >> 16) & ~w & 0xffff), (dim, lam)
            # without gw; the segment counts alone; in place
            gx3, none, _ = device.tv1_fibres_vjp_steps(steps, g, shape, dim)
            assert torch.equal(gx3, gx) and none is None
            _, _, nseg4 = device.tv1_fibres_vjp_steps(steps, None, shape, dim)
            assert torch.equal(nseg4, device.tv1_fibres_dof(y, dim)) and torch.equal(nseg4, nseg)
            gi = g.clone()
            out, _, _ = device.tv1_fibres_vjp_steps(steps, gi, shape, dim, out=gi)
            assert out is gi and torch.equal(gi, gx)
        if shape[dim] == 1:
            assert torch.equal(gx2, g)
        else:
            assert bool((gw2 == 0).all()) and int(nseg2.sum()) == fibres       # (lambda = 1e3 came last: one segment a fibre)


def test_fibre_level_bad_arguments(dev, clib):
    torch, device = dev.torch, dev.device
    y = dev.up(noise((16, 65)))
    steps = device.tv1_fibres_steps(y, 0)
    ns = np.array([16, 65], dtype=np.int32)
    assert clib.proxtv_tv1_steps_words(ns.ctypes.data, 2, 2) == -1 and b"dimension" in clib.proxtv_last_error()
    assert clib.proxtv_tv1_steps_words(np.array([0, 5], dtype=np.int32).ctypes.data, 2, 0) == 0
    with pytest.raises(ValueError):
        device.tv1_fibres_steps(y, 2)
    with pytest.raises(ValueError):
        device.tv1_fibres_vjp_steps(steps, y, (16, 65), 1)           # 65 words along 0, 80 along 1
    with pytest.raises(ValueError):
        device.tv1_fibres_vjp_steps(steps.double(), y, (16, 65), 0)
    with pytest.raises(ValueError):
        device.tv1_fibres_vjp_steps(steps, dev.up(noise((65, 16))), (16, 65), 0)
    gx = torch.full_like(y, 7.0)
    torch.cuda.synchronize()
    assert clib.proxtv_tv1_fibres_vjp_steps_dev(steps.data_ptr(), 0, gx.data_ptr(), 0, 0, ns.ctypes.data, 2, 0, 0) == 0
    assert b"g is required" in clib.proxtv_last_error() and bool((gx == 7.0).all())
    assert clib.proxtv_tv1_fibres_steps_dev(y.data_ptr(), y.data_ptr(), ns.ctypes.data, 2, 0, 0) == 0 and b"overlaps" in clib.proxtv_last_error()
    empty = device.tv1_fibres_steps(device.colmajor_empty((0, 5)), 0)
    assert empty.numel() == 0 and empty.dtype == torch.int32


# ---- 2. Douglas-Rachford -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maxit", [1, 35])
@pytest.mark.parametrize("shape", [(33, 18), (1, 40), (17, 1), (33, 18, 3)])
@pytest.mark.parametrize("weighted", [False, True])
def test_dr_steps_tape_gives_the_bits_of_the_outputs_tape(dev, shape, weighted, maxit):
    torch, device = dev.torch, dev.device
    U, g = dev.up(noise(shape, 2)), dev.up(noise(shape, 3))
    wc = wr = None
    if weighted:
        sc, sr = (max(shape[0] - 1, 0), shape[1]) + shape[2:], (shape[0], max(shape[1] - 1, 0)) + shape[2:]
        wc, wr = dev.up(0.3 * (0.5 + np.abs(noise(sc, 4)))), dev.up(0.3 * (0.5 + np.abs(noise(sr, 5))))
    kw = dict(max_iters=maxit, weights_col=wc, weights_row=wr, need_gw=True, need_y=True)
    a = device.dr2_vjp(U, g, 0.3, 0.45, **kw)
    b = device.dr2_vjp(U, g, 0.3, 0.45, tape="steps", **kw)
    c = device.dr2_vjp(U, g, 0.3, 0.45, tape="outputs", **kw)
    for name, x, y, z in zip(("gx", "gw_col", "gw_row", "glam", "y"), a, b, c):
        assert same(torch, x, y) and same(torch, x, z), name
    sums = device.dr2_vjp(U, g, 0.3, 0.45, max_iters=maxit, weights_col=wc, weights_row=wr, need_gw="sums", tape="steps")
    assert torch.equal(sums[0], a[0]) and np.array_equal(sums[3], a[3]) and sums[1] is None


def test_an_invalid_tape_is_refused_and_writes_nothing(dev, clib):
    torch, device = dev.torch, dev.device
    M, N = 6, 4
    U, g = dev.up(noise((M, N), 2)), dev.up(noise((M, N), 3))
    gU, s = torch.full_like(g, 7.0), torch.full_like(g, 7.0)
    glam = np.full(2, 7.0)
    ns, lams, dims = np.array([M, N], dtype=np.int32), np.full(2, 0.3), np.array([1.0, 2.0])
    torch.cuda.synchronize()
    for tape in (2, -1):
        assert clib.proxtv_DR2_TV_vjp_tape_dev(M, N, 1, U.data_ptr(), 0.5, 0.5, 0, 0, g.data_ptr(), s.data_ptr(), gU.data_ptr(), 0, 0,
                                               glam.ctypes.data, 3, tape, 0) == 0
        assert b"tape" in clib.proxtv_last_error()
        for which in (0, 1):
            assert clib.proxtv_PD_TV_vjp_tape_dev(which, U.data_ptr(), lams.ctypes.data, dims.ctypes.data, ns.ctypes.data, 2, 2, 3, g.data_ptr(),
                                                  s.data_ptr(), gU.data_ptr(), glam.ctypes.data, tape, 0) == 0
            assert b"tape" in clib.proxtv_last_error()
    assert bool((gU == 7.0).all()) and bool((s == 7.0).all()) and np.all(glam == 7.0)
    for bad in ("words", 1, None):
        with pytest.raises(ValueError):
            device.dr2_vjp(U, g, 0.5, tape=bad)
        with pytest.raises(ValueError):
            device.tvgen_vjp(U, g, [0.3, 0.3], [1, 2], 3, tape=bad)
    # ... and the same calls with tape = 1 go through
    assert clib.proxtv_DR2_TV_vjp_tape_dev(M, N, 1, U.data_ptr(), 0.5, 0.5, 0, 0, g.data_ptr(), s.data_ptr(), gU.data_ptr(), 0, 0,
                                           glam.ctypes.data, 3, 1, 0) == 1
    assert not bool((gU == 7.0).any()) and not bool((s == 7.0).any()) and not np.any(glam == 7.0)


# ---- 3. the Dykstra loops -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 7])
@pytest.mark.parametrize("shape", [(17, 15), (6, 18, 5), (1, 9)])
def test_pd_steps_tape_gives_the_bits_of_the_outputs_tape(dev, clib, shape, K):
    """pd2 with one and two terms, pd with one to four (the fourth shares the second's dimension)."""
    torch, device = dev.torch, dev.device
    x, g = dev.up(noise(shape, 6)), dev.up(noise(shape, 7))
    order = [1, 2, 3, 2] if len(shape) == 3 else [1, 2, 1, 2]
    lam = [0.1, 0.35, 0.2, 0.15]
    for method, terms in (("pd2", (1, 2)), ("pd", (1, 2, 3, 4))):
        for P in terms:
            a = device.tvgen_vjp(x, g, lam[:P], order[:P], K, method, need_glam=True, need_y=True)
            b = device.tvgen_vjp(x, g, lam[:P], order[:P], K, method, need_glam=True, need_y=True, tape="steps")
            for name, u, v in zip(("gx", "glam", "y"), a, b):
                assert same(torch, u, v), (method, P, name)
            # gy is g
            gi = g.clone()
            ns, lams = np.array(shape, dtype=np.int32), np.array(lam[:P]) * (P if method == "pd" else 1)
            dims = np.array(order[:P], dtype=np.float64)
            torch.cuda.synchronize()
            assert clib.proxtv_PD_TV_vjp_tape_dev(0 if method == "pd2" else 1, x.data_ptr(), lams.ctypes.data, dims.ctypes.data, ns.ctypes.data,
                                                  len(shape), P, K, gi.data_ptr(), 0, gi.data_ptr(), 0, 1, 0) == 1
            assert torch.equal(gi, a[0]), (method, P)


# ---- 4. autograd ---------------------------------------------------------------------------------------------------------------------------
def grads(torch, f, tensors, cot):
    ts = [t.clone().requires_grad_(True) for t in tensors]
    y = f(*ts)
    (cot * y).sum().backward()
    return y.detach(), [t.grad for t in ts]


def test_autograd_with_the_steps_tape(dev, clib):
    from proxtv_amd import autograd
    torch = dev.torch
    shape = (20, 26)
    x, cot = dev.up(noise(shape, 8)), dev.up(noise(shape, 9))
    w = torch.tensor(0.3, dtype=torch.float64, device="cuda")
    wc, wr = dev.up(0.3 * (0.5 + np.abs(noise((19, 26), 4)))), dev.up(0.3 * (0.5 + np.abs(noise((20, 25), 5))))
    xs, cots = dev.up(noise(shape + (3,), 8)), dev.up(noise(shape + (3,), 9))
    vol, cotv = dev.up(noise(shape + (14,), 8)), dev.up(noise(shape + (14,), 9))
    ws = [torch.tensor(v, dtype=torch.float64, device="cuda") for v in (0.1, 0.2, 0.15)]
    cases = (
        ("tv1_fibres", lambda tape: (lambda a, b: autograd.tv1_fibres(a, b, 1, tape=tape)), (x, w), cot),
        ("tv1_fibres weighted", lambda tape: (lambda a, b: autograd.tv1_fibres(a, 0.0, 0, weights=b, tape=tape)), (x, wc), cot),
        ("tv1_2d", lambda tape: (lambda a, b: autograd.tv1_2d(a, b, tape=tape)), (x, w), cot),
        ("tv1w_2d", lambda tape: (lambda a, b, c: autograd.tv1w_2d(a, b, c, tape=tape)), (x, wc, wr), cot),
        ("tv1_2d_batch", lambda tape: (lambda a, b: autograd.tv1_2d_batch(a, b, tape=tape)), (xs, w), cots),
        ("tvgen pd", lambda tape: (lambda a, b, c, d: autograd.tvgen(a, [b, c, d], [1, 2, 3], tape=tape)), (vol, *ws), cotv),
        ("tvgen pd2", lambda tape: (lambda a, b, c: autograd.tvgen(a, [b, c], [1, 3], tape=tape)), (vol, *ws[:2]), cotv),
    )
    for name, make, tensors, c in cases:
        y0, g0 = grads(torch, make("outputs"), tensors, c)
        y1, g1 = grads(torch, make("steps"), tensors, c)
        assert torch.equal(y0, y1), name
        for a, b in zip(g0, g1):
            assert a is not None and torch.equal(a, b), name
        with pytest.raises(ValueError):
            make("words")(*tensors)
    # what the graph keeps of a fibre prox: the words, not y
    xt = x.clone().requires_grad_(True)
    y = autograd.tv1_fibres(xt, 0.3, 1, tape="steps")
    (saved,) = y.grad_fn.saved_tensors
    ns = np.array(shape, dtype=np.int32)
    assert saved.dtype == torch.int32 and saved.numel() == clib.proxtv_tv1_steps_words(ns.ctypes.data, 2, 1) == 20 * 2
    y = autograd.tv1_fibres(xt, 0.3, 1)
    (saved,) = y.grad_fn.saved_tensors
    assert saved.dtype == torch.float64 and tuple(saved.shape) == shape


# ---- 5. the cap ----------------------------------------------------------------------------------------------------------------------------
def test_under_a_cap_that_refuses_the_outputs_the_steps_tape_goes_through(clib):
    """PROXTV_POOL_CAP_MB is read once per process: a fresh child with a 1 MiB cap (tests/vjp_steps_cap_child.py) is refused the 5.76 MB
    of sweep outputs of a 100 x 100 image, runs the same call on 361 600 B of step codes and live arrays, and prints the sha1 of what
    came out; here the same inputs go through tape = 0 at the default cap.  The same for the two Dykstra loops."""
    import vjp_steps_cap_child as child
    env = dict(os.environ, PROXTV_POOL_CAP_MB="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "vjp_steps_cap_child.py")], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "CAP_CHILD_OK" in r.stdout
    lines = {line.split()[0]: line.split()[1:] for line in r.stdout.splitlines() if line.split() and line.split()[0] in ("DR", "PD0", "PD1")}
    rc, gU, s, glam = child.dr(clib, 100, 100, 0)
    assert rc == 1 and lines["DR"] == [child.sha(gU), child.sha(s), child.sha(glam)]
    for which, npen in child.PD_CASES:
        rc, gy, x, glam = child.pd(clib, which, npen, 100, 100, 0)
        assert rc == 1 and lines[f"PD{which}"] == [child.sha(gy), child.sha(x), child.sha(glam)]
