"""The TV-Lp fibre prox for general p on the device (csrc/tvp.hip) and its way through every solver behind option general_p.

Yardsticks: tests/tvp_model.py (the duality gap of ANY x, in plain numpy) and the compiled reference's outputs in
tests/golden/golden_pgen.npz.  Every bound is an argument, none a measurement: P is 1-strongly convex, so an output with gap g lies
within sqrt(2 g) of the minimiser, and two outputs within the sum of their radii."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tvp_model as tm
from conftest import load_golden

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LOOP_BOUND = 4 * np.sqrt(2e-5)     # test_oracle_p2.py's bar for the splitting loops when the fibre prox is inexact


@pytest.fixture(scope="module")
def gpg():
    return load_golden("golden_pgen.npz")


@pytest.fixture(scope="module")
def dev(ptv):
    import torch
    from proxtv_amd import device

    class Dev:
        def up(self, a):
            return device.to_colmajor(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda())

        def fibres(self, a, w, p, dim, gap=False):
            r = device.tvp_fibres(self.up(a), w, p, dim, return_gap=gap)
            return (r[0].cpu().numpy(), r[1].cpu().numpy()) if gap else r.cpu().numpy()
    d = Dev()
    d.device, d.torch = device, torch
    return d


@pytest.fixture
def general(ptv):
    """option general_p on for one test, restored afterwards"""
    before = ptv.general_p(True)
    try:
        yield ptv
    finally:
        ptv.general_p(before)


def counter(clib, name):
    return clib.proxtv_debug_counter(name.encode())


def check_case(x, gap, y, lam, p):
    n = y.size
    scale, pmean = max(1.0, np.abs(y).max()), tm.primal(np.full(n, y.mean()), y, lam, p)
    model = tm.tvp_gap(x, y, lam, p)
    print(f"n={n} p={p} lam={lam}: gap {gap:.3e} model {model:.3e}")
    assert model <= 1e-5, (n, p, lam, model)
    assert abs(x.mean() - y.mean()) <= 1e-12 * scale
    assert abs(gap - model) <= 0.1 * model + 1e-10 * max(1.0, pmean), (n, p, lam, gap, model)


def test_gap_of_the_fibre_prox_over_the_golden_grid(dev, clib, gpg):
    capped, solved = counter(clib, "tvp_capped"), counter(clib, "tvp_fibres")
    for k, (n, p, lam) in enumerate(tm.GRID):
        y = gpg[f"y_{int(n)}"]
        x, gap = dev.fibres(y, lam, p, 0, gap=True)
        check_case(x, float(gap), y, lam, p)
    assert counter(clib, "tvp_capped") == capped
    assert 0 < counter(clib, "tvp_fibres") - solved <= len(tm.GRID)


def test_gap_of_tvp_1d_and_its_info_over_the_golden_grid(general, clib, gpg):
    capped = counter(clib, "tvp_capped")
    for k, (n, p, lam) in enumerate(tm.GRID):
        y = np.ascontiguousarray(gpg[f"y_{int(n)}"])
        x, info = np.zeros(y.size), np.full(3, -1.0)
        assert clib.TV(y.ctypes.data, lam, x.ctypes.data, info.ctypes.data, y.size, p, None) == 1
        check_case(x, info[1], y, lam, p)
        assert info[2] == 0 and info[0] >= 0
        if k % 7 == 0:      # the Python surface and the other symbols are the same solver: the same bits
            for method in ("gp", "fw", "gpfw"):
                assert np.array_equal(general.tvp_1d(y, lam, p, method=method), x)
    assert counter(clib, "tvp_capped") == capped


def test_reference_within_the_two_gaps(dev, gpg):
    for k, (n, p, lam) in enumerate(tm.GRID):
        y, ref = gpg[f"y_{int(n)}"], gpg[f"x_{k}"]
        got = dev.fibres(y, lam, p, 0)
        bound = tm.radius(got, y, lam, p) + tm.radius(ref, y, lam, p) + 1e-12 * max(1.0, np.abs(y).max())
        assert np.linalg.norm(got - ref) <= bound, (n, p, lam, np.linalg.norm(got - ref), bound)


@pytest.mark.parametrize("shape,dims", [((37, 70, 3), (0, 1, 2)), ((9, 130), (0, 1))])
def test_geometry_every_fibre_is_its_own_call_bit_for_bit(dev, shape, dims):
    p, lam = 3.0, 0.8
    a = np.random.default_rng(11).standard_normal(shape)
    a[shape[0] // 2:] += 2.0
    for dim in dims:
        got, gap = dev.fibres(a, lam, p, dim, gap=True)
        again, gap2 = dev.fibres(a, lam, p, dim, gap=True)
        assert np.array_equal(got, again) and np.array_equal(gap, gap2)
        rest = [s for i, s in enumerate(shape) if i != dim]
        assert gap.shape == tuple(rest) and gap.max() <= 1e-5
        # the fibres as rows of one (len, count) array, then a sample of them one by one: corners, wave boundaries, a spread
        fib = np.moveaxis(a, dim, 0).reshape(shape[dim], -1, order="F")
        gfib, ggap = np.moveaxis(got, dim, 0).reshape(shape[dim], -1, order="F"), gap.reshape(-1, order="F")
        count = fib.shape[1]
        for j in sorted({0, 1, 63, 64, 65, 127, 128, 129, count - 1} & set(range(count)) | set(range(0, count, 17))):
            one, g1 = dev.fibres(fib[:, j], lam, p, 0, gap=True)
            assert np.array_equal(one, gfib[:, j]), (dim, j)
            assert float(g1) == ggap[j]


def test_closed_forms(dev, clib):
    solved = counter(clib, "tvp_fibres")
    y = tm.signal(17, 2)
    for p in (1.5, 3.0):
        x, gap = dev.fibres(y[:1], 1.0, p, 0, gap=True)
        assert np.array_equal(x, y[:1]) and float(gap) == 0
        x, gap = dev.fibres(y, 0.0, p, 0, gap=True)
        assert np.array_equal(x, y) and float(gap) == 0
        x, gap = dev.fibres(y, 1e6, p, 0, gap=True)
        assert np.abs(x - y.mean()).max() <= 1e-12 * max(1.0, np.abs(y).max()) and float(gap) == 0
        x = dev.fibres(np.full((9, 5), 0.3), 0.5, p, 0)
        assert np.array_equal(x, np.full((9, 5), 0.3))
        x = dev.fibres(np.arange(12.0).reshape(1, 12), 0.5, p, 0)          # a dimension of extent 1
        assert np.array_equal(x, np.arange(12.0).reshape(1, 12))
    assert counter(clib, "tvp_fibres") == solved


def test_dispatch_p1_p2_are_the_exact_solvers_and_the_range_is_checked(dev):
    a = np.random.default_rng(5).standard_normal((33, 70))
    x = dev.up(a)
    for dim in (0, 1):
        y1, gap = dev.device.tvp_fibres(x, 0.4, 1, dim, return_gap=True)
        assert dev.torch.equal(y1, dev.device.tv1_fibres(x, 0.4, dim)) and float(gap.abs().max()) == 0
        y2, gap = dev.device.tvp_fibres(x, 0.4, 2, dim, return_gap=True)
        assert dev.torch.equal(y2, dev.device.tv2_fibres(x, 0.4, dim)) and float(gap.abs().max()) == 0
    for p in (1.001, 100, np.inf, 0.5):
        with pytest.raises(NotImplementedError):
            dev.device.tvp_fibres(x, 0.4, p, 1)


def test_the_c_entry_point_reports_an_out_of_range_norm(dev, clib):
    x = dev.up(np.random.default_rng(5).standard_normal((8, 6)))
    out = dev.torch.full_like(x, 7.0)
    ns = np.array([8, 6], dtype=np.int32)
    dev.torch.cuda.synchronize()
    for p in (1.001, 100.0, float("inf")):
        assert clib.proxtv_tvpg_fibres_dev(x.data_ptr(), out.data_ptr(), 0, ns.ctypes.data, 2, 1, 0.4, p, 0) == 0
        assert b"1.002 < p < 100" in clib.proxtv_last_error() and bool((out == 7.0).all())
    assert clib.proxtv_tvpg_fibres_dev(x.data_ptr(), out.data_ptr(), 0, ns.ctypes.data, 2, 1, 0.4, 3.0, 0) == 1
    assert clib.proxtv_last_error() == b"" and not bool((out == 7.0).any())


def test_opt_in(ptv, clib, dev):
    from proxtv_amd import autograd
    y = np.ascontiguousarray(tm.signal(17, 3))
    x, info = np.full(17, 7.0), np.zeros(3)
    img = dev.up(np.random.default_rng(2).standard_normal((8, 6)))
    before = ptv.general_p(False)
    try:
        with pytest.raises(NotImplementedError):
            ptv.tvp_1d(y, 0.5, 1.5)
        assert clib.TV(y.ctypes.data, 0.5, x.ctypes.data, info.ctypes.data, 17, 3.0, None) == 0
        assert info[2] == 3 and (x == 7.0).all()
        with pytest.raises(NotImplementedError):
            dev.device.tvp_2d(img, 0.3, 0.3, 1.5, 1)
        with pytest.raises(NotImplementedError):
            dev.device.tvgen(img, [0.3, 0.3], [1, 2], ps=[3, 1])
        assert ptv.general_p(True) is False
        got = ptv.tvp_1d(y, 0.5, 1.5)
        assert tm.tvp_gap(got, y, 0.5, 1.5) <= 1e-5
        assert clib.TV(y.ctypes.data, 0.5, x.ctypes.data, info.ctypes.data, 17, 3.0, None) == 1
        assert info[2] == 0 and tm.tvp_gap(x, y, 0.5, 3.0) <= 1e-5
        for p in (1.001, 100.0, np.inf):       # beyond the general solver's range: refused either way
            with pytest.raises(NotImplementedError):
                ptv.tvp_1d(y, 0.5, p)
            assert clib.TV(y.ctypes.data, 0.5, x.ctypes.data, info.ctypes.data, 17, p, None) == 0 and info[2] == 3
        for on in (True, False):               # the derivatives refuse whatever the option says
            ptv.general_p(on)
            with pytest.raises(NotImplementedError):
                dev.device.dr2_vjp(img, img, 0.3, p_col=1.5)
            with pytest.raises(NotImplementedError):
                dev.device.tvgen_vjp(img, img, [0.3, 0.3], [1, 2], 3, ps=[1.5, 1])
            with pytest.raises(NotImplementedError):
                autograd.tvgen(img, [0.3, 0.3], [1, 2], ps=[1.5, 1])
            with pytest.raises(NotImplementedError):
                dev.device.tvgen(img, [0.3, 0.3], [1, 2], method="pdr", ps=[1.5, 1])
    finally:
        ptv.general_p(before)


def test_loops_against_the_reference(general, dev, gpg):
    img, vol = gpg["img"], gpg["vol"]
    w = gpg["img_w"]
    for j, (p1, p2) in enumerate(gpg["img_norms"]):
        for tag, iters in (("5", 5), ("0", 0)):
            got = general.tvp_2d(img, w[0], w[1], p1, p2, max_iters=iters)
            err = np.abs(got - gpg[f"dr2_{tag}_{j}"]).max()
            print(f"dr2 norms ({p1}, {p2}) max_iters {iters}: {err:.3e}")
            assert err <= LOOP_BOUND, (p1, p2, iters, err)
            y, info = dev.device.tvgen(dev.up(img), list(w), [1, 2], max_iters=iters, ps=[p1, p2])
            err = np.abs(y.cpu().numpy() - gpg[f"pd2_{tag}_{j}"]).max()
            print(f"pd2 norms ({p1}, {p2}) max_iters {iters}: {err:.3e}, {info[0]} iterations (reference {gpg[f'pd2_{tag}_{j}_info'][0]})")
            assert err <= LOOP_BOUND, (p1, p2, iters, err)
            if iters == 5:
                assert info[0] == gpg[f"pd2_5_{j}_info"][0]
        got = general.tvgen(img, np.array(w), [1, 2], [p1, p2])          # the host surface: PD2_TV
        assert np.abs(got - gpg[f"pd2_0_{j}"]).max() <= LOOP_BOUND
    got = general.tvgen(vol, np.array(gpg["vol_w"]), [int(d) for d in gpg["vol_dims"]], gpg["vol_norms"])
    err = np.abs(got - gpg["pd_vol"]).max()
    print(f"pd on the volume: {err:.3e}")
    assert err <= LOOP_BOUND


def test_scratch_beyond_the_pool_cap_is_refused():
    """PROXTV_POOL_CAP_MB is read once per process: a fresh child with a 1 MiB cap."""
    env = dict(os.environ, PROXTV_POOL_CAP_MB="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "tvp_cap_child.py")], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "CAP_CHILD_OK" in r.stdout
