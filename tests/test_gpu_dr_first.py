"""The first row sweep of a Douglas-Rachford solve reads its two constant operands (t0 = 2 mean(U) per image and s' = -t0) from a
table (option dr_first = 1, the default; ops.hpp: OP_DR_ROW_FIRST) instead of two arrays filled with them (dr_first = 0).  Same
operation order, so every result must be the same bits and every info the same numbers, on every path the sweep can take."""
import numpy as np
import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu


def _dev(a):
    from proxtv_amd import device
    return device.to_colmajor(torch.from_numpy(np.ascontiguousarray(a)).cuda())


def _both(clib, solve, knobs=()):
    """solve() under dr_first = 1 and again under dr_first = 0 (other knobs as given): ((y, info), (y, info))."""
    before = [(k, clib.proxtv_set_option(k, v)) for k, v in knobs]
    first = clib.proxtv_set_option(b"dr_first", 1)
    try:
        res = []
        for v in (1, 0):
            clib.proxtv_set_option(b"dr_first", v)
            y, info = solve()
            torch.cuda.synchronize()
            res.append((y.clone(), np.array(info, dtype=np.float64).copy()))
        return res
    finally:
        clib.proxtv_set_option(b"dr_first", first)
        for k, v in reversed(before):
            clib.proxtv_set_option(k, v)


def _same(res, what):
    (y1, i1), (y0, i0) = res
    assert torch.equal(y1, y0), f"{what}: dr_first 1 and 0 differ in {int((y1 != y0).sum())} elements"
    assert np.array_equal(i1, i0), (what, i1, i0)


# 40 x 300: rows of 300 samples in 40 fibres -- not a multiple of the 32-fibre tile, three 128-sample blocks (links across workgroups,
# halo rows) ; 33 x 130: one fibre past a tile, two samples past a block ; 96 x 96: the one-block (SHORT) geometry ; 2 x 20000
@pytest.mark.parametrize("shape", [(40, 300), (33, 130), (96, 96), (2, 20000)])
@pytest.mark.parametrize("lam", [0.1, 1.0])
def test_first_row_sweep_same_bits(ptv, clib, shape, lam):
    from proxtv_amd import device
    X = _dev(np.random.default_rng(shape[0] * 1000 + shape[1]).standard_normal(shape) + 0.75)
    _same(_both(clib, lambda: device.tv1_2d(X, lam)), f"{shape} lambda {lam}")


@pytest.mark.parametrize("rung", [0, 1, 3])
@pytest.mark.parametrize("lam", [0.1, 1.0])
def test_first_row_sweep_pinned_rungs(ptv, clib, rung, lam):
    """Rungs 0 and 1: the plain and the robust tile (on rung 1 the unweighted solve takes the OP_DR_COL_V form, which keeps its own first
    iteration; dr_form = 0 puts the new sweep on the robust tile too).  Rung 3: transposed copies and the pinning solver, where the
    arrays are filled as before."""
    from proxtv_amd import device
    X = _dev(np.random.default_rng(7 + rung).standard_normal((40, 300)) - 1.5)
    for form in (1, 0):
        _same(_both(clib, lambda: device.tv1_2d(X, lam), knobs=((b"chunk_mode", rung), (b"dr_form", form))), f"rung {rung} form {form} lambda {lam}")


def test_first_row_sweep_batch_takes_each_image_its_own_constant(ptv, clib):
    from proxtv_amd import device
    rng = np.random.default_rng(11)
    xs = np.stack([rng.standard_normal((40, 300)) + m for m in (-5.0, 0.0, 7.0)], axis=2)
    Xs = _dev(xs)
    res = _both(clib, lambda: device.tv1_2d_batch(Xs, 0.2))
    _same(res, "batch")
    # ... and the constant of its own image: every image of the batch is the bits of its single-image solve
    for b in range(3):
        y, _ = device.tv1_2d(_dev(xs[:, :, b]), 0.2)
        assert torch.equal(res[0][0][:, :, b], y), f"image {b}"


@pytest.mark.parametrize("rung", [-1, 0, 1])
def test_first_row_sweep_weighted(ptv, clib, rung):
    from proxtv_amd import device
    rng = np.random.default_rng(13)
    X = _dev(rng.standard_normal((40, 300)) + 2.0)
    W1, W2 = _dev(rng.uniform(0.05, 0.15, (39, 300))), _dev(rng.uniform(0.05, 0.15, (40, 299)))
    _same(_both(clib, lambda: device.tv1w_2d(X, W1, W2), knobs=((b"chunk_mode", rung),)), f"weighted rung {rung}")


@pytest.mark.parametrize("maxit", [1, 7])
def test_first_row_sweep_iteration_counts_through_the_c_abi(clib, maxit):
    X = np.asfortranarray(np.random.default_rng(17).standard_normal((40, 300)) + 3.0)

    def call():
        out, info = np.zeros(X.shape, order="F"), np.array([-7.0, -7.0, -7.0])
        rc = clib.DR2_TV(X.shape[0], X.shape[1], X.ctypes.data, 0.3, 0.3, 1.0, 1.0, out.ctypes.data, 1, maxit, info.ctypes.data)
        assert rc == 0 and info[0] == maxit
        return out, info

    first = clib.proxtv_set_option(b"dr_first", 1)
    try:
        y1, i1 = call()
        clib.proxtv_set_option(b"dr_first", 0)
        y0, i0 = call()
    finally:
        clib.proxtv_set_option(b"dr_first", first)
    assert np.array_equal(y1, y0) and np.array_equal(i1, i0)


def test_first_row_sweep_against_the_reference(ptv, clib, g2d):
    """The reference's own output (the fixture), at the tolerance of the parity tests, with the option on -- and stated, not assumed."""
    first = clib.proxtv_set_option(b"dr_first", 1)
    try:
        for name in g2d["names"]:
            X, lam = g2d[f"{name}/X"], float(g2d[f"{name}/lam"])
            assert_close(ptv.tv1_2d(X, lam), g2d[f"{name}/dr2"], what=f"{name}:dr2")
            assert_close(ptv.tv1w_2d(X, g2d[f"{name}/W1"], g2d[f"{name}/W2"]), g2d[f"{name}/dr2w"], what=f"{name}:dr2w")
    finally:
        clib.proxtv_set_option(b"dr_first", first)
