"""The along-fibre kernel's segment with the fibre's last sample (sweep_along_kernel `endseg`: staged with clamped rows, rebuilt with a
row count per lane, streamed out in whole groups of 64 rows plus one tested group) on the GPU.

Column sweeps through device.tv1_fibres(..., dim=0) and small DR solves on M x 8 images, M chosen so that the end segment takes every
shape the kernel distinguishes with 17-sample chunks and 1088-sample segments; against the CPU oracle's fibre prox, against the same
call with option "runs" off, and twice for bit-reproducibility."""
import numpy as np
import pytest

from conftest import assert_close

pytestmark = pytest.mark.gpu

# an end segment of one sample; around the edge of `interior` (seg_s + SEG + T <= len - 1); exactly one whole chunk; a whole chunk and a
# partial one; ending exactly on a segment, and one more; a whole-chunk boundary; around the chunk boundary next to 4096's own partial
# last chunk; the workload's own shape, and one more; four full segments; five segments
LENGTHS = (1089, 1096, 1097, 1098, 1105, 1110, 2176, 2177, 3264 + 17, 4079, 4080, 4081, 4096, 4097, 4352, 5000)


@pytest.fixture(scope="module")
def dev(ptv):
    import torch
    from proxtv_amd import device

    class Dev:
        pass
    d = Dev()
    d.device = device
    d.up = lambda a: device.to_colmajor(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    return d


def columns(dev, X, lam, weights=None):
    w = None if weights is None else dev.up(weights)
    return dev.device.tv1_fibres(dev.up(X), lam, 0, weights=w).cpu().numpy()


def families(M, N, seed):
    """(name, image, penalty): unit noise in the known-runs regime and in the speculative one, a long last piece that runs into the free
    end, integer ties."""
    rng = np.random.default_rng(seed)
    yield "noise 0.1", rng.standard_normal((M, N)), 0.1
    yield "noise 0.3", rng.standard_normal((M, N)), 0.3
    X = rng.standard_normal((M, N))
    X[-40:] = X[-40]
    yield "constant tail", X, 0.1
    yield "integer ties", rng.integers(-2, 3, (M, N)).astype(float), 0.25


def check_columns(dev, clib, oracle, X, lam, what):
    got = columns(dev, X, lam)
    want = np.apply_along_axis(lambda f: oracle.tv1_hybrid(np.ascontiguousarray(f), lam), 0, X)
    assert_close(got, want, tol=1e-12, what=what)
    before = clib.proxtv_set_option(b"runs", 0)
    try:
        plain = columns(dev, X, lam)
    finally:
        clib.proxtv_set_option(b"runs", before)
    assert_close(got, plain, tol=1e-13, what=what + ", against the same call without known runs")
    assert np.array_equal(got, columns(dev, X, lam)), what + ": two calls differ"


@pytest.mark.parametrize("M", LENGTHS)
def test_column_sweeps_of_every_end_segment_shape(dev, clib, oracle, M):
    for name, X, lam in families(M, 8, M):
        check_columns(dev, clib, oracle, X, lam, f"{M} x 8, {name}")


def test_a_workgroup_with_segments_of_two_fibres(dev, clib, oracle):
    for name, X, lam in families(4096, 3, 5):
        check_columns(dev, clib, oracle, X, lam, f"4096 x 3, {name}")


@pytest.mark.parametrize("rung", (0, 1))
def test_pinned_rungs(dev, clib, oracle, rung):
    """Whatever the policy makes of these small images, the plain and the robust instantiation both meet every family: the rung pinned."""
    before = clib.proxtv_set_option(b"chunk_mode", rung)
    try:
        for M in (1110, 2177, 4096):
            for name, X, lam in families(M, 8, 100 + M):
                check_columns(dev, clib, oracle, X, lam, f"rung {rung}, {M} x 8, {name}")
    finally:
        clib.proxtv_set_option(b"chunk_mode", before)


@pytest.mark.parametrize("M", (4096, 2177))
def test_dr_solves(ptv, oracle, M):
    X = np.random.default_rng(M).standard_normal((M, 8))
    got = ptv.tv1_2d(X, 0.1)
    assert_close(got, oracle.dr2(X, 0.1)[0], tol=1e-9, what=f"dr2 {M} x 8")
    assert np.array_equal(got, ptv.tv1_2d(X, 0.1))


def test_weighted_column_sweep(dev, oracle):
    """The nine-sample instantiation: eight segments of 576 samples, the last one 64 samples long."""
    rng = np.random.default_rng(6)
    X = rng.standard_normal((4096, 8))
    W = rng.uniform(0.05, 0.15, (4095, 8))
    got = columns(dev, X, 0.0, weights=W)
    want = np.stack([oracle.tv1_weighted(np.ascontiguousarray(X[:, j]), np.ascontiguousarray(W[:, j])) for j in range(8)], axis=1)
    assert_close(got, want, tol=1e-12, what="weighted columns 4096 x 8")
    assert np.array_equal(got, columns(dev, X, 0.0, weights=W))
