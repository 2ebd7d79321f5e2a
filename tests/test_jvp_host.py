"""The tangent load of the forward-mode fibre derivative without a GPU: the functions the HIP kernels run (proxtv_amd/csrc/jvpcore.hpp on
top of vjpcore.hpp), compiled for the host by tests/jvp_host.cpp and driven chunk by chunk, against the numpy model of tests/jvp_model.py.
Both forms of the edge-injection term -- from a chunk's masks (the strided kernel) and from a sample's neighbours (the contiguous kernel's
staging loop) -- for chunks of 1, 2, 7 and 16 samples and fibres of 1, 2, 15, 16, 17, 33 and 1041, with steps that fall on chunk
boundaries and boundaries that are no steps.  Tolerance: the certifier's rounding rule, 64 n 2^-52 max|v|, v the model's."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import jvp_model as jm
import vjp_model as vm

HERE = os.path.dirname(os.path.abspath(__file__))
CHUNKS = (1, 2, 7, 16)
LENGTHS = (1, 2, 15, 16, 17, 33, 1041)


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(tempfile.mkdtemp(prefix="ptv_jvp_"), "libjvp_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "jvp_host.cpp")],
                   check=True)
    lib = C.CDLL(out)
    lib.jvp_host_run.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_double, C.c_void_p, C.c_double, C.c_void_p, C.c_double,
                                 C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return lib


def run(lib, y, arrays, dw, dlam, chunk, staged, inject=1, out=None):
    """arrays: up to three (array | None, coefficient)."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    arrays = list(arrays) + [(None, 0.0)] * (3 - len(arrays))
    dy = np.full(y.size, np.nan) if out is None else out
    args = []
    for a, c in arrays:
        args += [None if a is None else a.ctypes.data, float(c)]
    rc = lib.jvp_host_run(y.ctypes.data, *args, None if dw is None else dw.ctypes.data, float(dlam), inject, y.size, chunk, staged,
                          dy.ctypes.data)
    assert rc == 0, chunk
    return dy


def fibres(oracle):
    """(name, y): proxes of unit noise (lambda 0.1 / 0.5 and per-edge U(0.05, 0.5)) at every length, plus staircases whose steps sit
    exactly on the boundaries of chunks of 1, 2, 7 and 16 samples, up and down, and a flat fibre, where no boundary is a step."""
    rng = np.random.default_rng(2027)
    for n in LENGTHS:
        x = rng.standard_normal(n)
        for lam in (0.1, 0.5):
            yield f"n{n} lam{lam}", x.copy() if n == 1 else oracle.tv1_linearized(x, lam)
        if n >= 2:
            yield f"n{n} weighted", oracle.tv1_weighted(x, rng.uniform(0.05, 0.5, n - 1))
    levels = np.repeat(rng.standard_normal(10), 112)[:1041]      # steps at multiples of 112 = lcm(1, 2, 7, 16)
    yield "steps at chunk boundaries", levels
    yield "steps at chunk boundaries, monotone down", -np.repeat(np.arange(10.0), 112)[:1041]
    yield "flat", np.full(1041, 0.75)
    yield "every edge a step", np.cumsum(rng.uniform(0.1, 1.0, 33)) * np.where(np.arange(33) % 2, 1.0, -1.0)


def test_chunked_tangent_load_equals_the_model(harness, oracle):
    rng = np.random.default_rng(31)
    worst = 0.0
    for name, y in fibres(oracle):
        vm.assert_unambiguous(y)
        n = y.size
        dx, b, c = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
        dw = rng.uniform(-1.0, 1.0, max(n - 1, 0))
        edges = np.ones(max(n - 1, 0))
        for what, arrays, ddw, dlam in (("dx", [(dx, 1.0)], None, 0.0), ("dlam", [], None, 0.7), ("dw", [(None, 0.0)], dw, 0.0),
                                        ("all", [(dx, 1.0), (b, -1.0), (c, 2.0)], dw, -0.3), ("no dU", [(None, 1.0), (b, -1.0), (c, 2.0)], dw, 0.0)):
            comb = sum((coef * a for a, coef in arrays if a is not None), np.zeros(n))
            dr = (ddw if ddw is not None else 0.0 * edges) + dlam * edges
            want, v = jm.jvp_1d(y, comb, dr)
            bound = vm.rounding_bound(n, v)
            first = None
            for chunk in CHUNKS:
                for staged in (0, 1):
                    dy = run(harness, y, arrays, ddw, dlam, chunk, staged)
                    err = float(np.max(np.abs(dy - want)))
                    worst = max(worst, err / bound if bound > 0 else 0.0)
                    assert err <= bound, (name, what, chunk, staged, err, bound)
                    if staged == 0:
                        first = dy
                    else:
                        assert np.array_equal(dy, first), (name, what, chunk, "the two forms of E differ")
                    assert np.all(np.diff(dy)[~vm.steps(y)] == 0.0), (name, what, chunk)       # a segment has one value, bit for bit
    print(f"host harness: worst error / bound {worst:.3f}")


def test_in_place_zero_and_no_injection(harness, oracle):
    rng = np.random.default_rng(32)
    y = oracle.tv1_linearized(rng.standard_normal(200), 0.3)
    dx = rng.standard_normal(200)
    for chunk in CHUNKS:
        for staged in (0, 1):
            plain = run(harness, y, [(dx, 1.0)], None, 0.0, chunk, staged)
            # dr = 0 with and without the injection pass: the same values; without it, the segmented mean of vjp_host's
            assert np.array_equal(run(harness, y, [(dx, 1.0)], None, 0.0, chunk, staged, inject=0), plain)
            assert np.max(np.abs(plain - vm.vjp_1d(y, dx)[0])) <= vm.rounding_bound(200, dx)
            buf = dx.copy()
            assert np.array_equal(run(harness, y, [(buf, 1.0)], None, 0.5, chunk, staged, out=buf), run(harness, y, [(dx, 1.0)], None, 0.5, chunk, staged))
            assert np.array_equal(run(harness, y, [], None, 0.0, chunk, staged), np.zeros(200))
