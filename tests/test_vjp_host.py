"""The derivative of the 1-D TV-L1 prox without a GPU: (a) the closed form (tests/vjp_model.py) against central differences of the
CPU oracle, (b) the chunk-level functions the HIP kernels run (proxtv_amd/csrc/vjpcore.hpp), compiled for the host by
tests/vjp_host.cpp, against that model."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import vjp_model as vm

HERE = os.path.dirname(os.path.abspath(__file__))
CHUNKS = (1, 2, 7, 64)


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(tempfile.mkdtemp(prefix="ptv_vjp_"), "libvjp_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "vjp_host.cpp")],
                   check=True)
    lib = C.CDLL(out)
    lib.vjp_host_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.vjp_host_step_rule.argtypes = [C.c_void_p]
    lib.vjp_host_is_step.argtypes = [C.c_double, C.c_double]
    return lib


def run(lib, y, g, chunk, want_gw=True, inplace=False):
    y = np.ascontiguousarray(y, dtype=np.float64)
    g = np.array(g, dtype=np.float64)
    gx = g if inplace else np.full(y.size, np.nan)
    gw = np.full(max(y.size - 1, 0), np.nan)
    nseg = lib.vjp_host_run(y.ctypes.data, g.ctypes.data, y.size, chunk, gx.ctypes.data, gw.ctypes.data if want_gw else None)
    assert nseg >= 0, chunk
    return gx, gw, nseg


# ---- (a) the closed form against the oracle ----------------------------------------------------------------------------------------
def test_closed_form_equals_central_differences_of_the_oracle(oracle):
    """gx = P c and gw against central differences (h = 1e-5) of c . prox, uniform lambda (oracle.tv1_hybrid) and per-edge weights
    (oracle.tv1_weighted): within 1e-8.  Differences for n <= 129 (per-edge gw: n <= 65); every case checks the precondition and
    what the closed form must satisfy whatever n (P symmetric and idempotent, trace P = segments)."""
    worst = 0.0
    for n, lam, x, c, w in vm.cases():
        for weighted in (False, True):
            if weighted and n < 2:
                continue
            prox = (lambda v, ww=w: oracle.tv1_weighted(v, ww)) if weighted else (lambda v, ll=lam: oracle.tv1_hybrid(v, ll))
            y = prox(x)
            vm.assert_unambiguous(y)
            gx, gw, nseg = vm.vjp_1d(y, c)
            assert nseg == 1 + int(np.count_nonzero(np.diff(y)))
            again = vm.vjp_1d(y, gx)[0]
            assert np.max(np.abs(again - gx)) <= vm.rounding_bound(n, c)                      # P P = P
            other = np.cos(np.arange(n))
            assert abs(np.dot(other, gx) - np.dot(vm.vjp_1d(y, other)[0], c)) <= 4 * vm.rounding_bound(n, c) * n ** 0.5   # P = P^T
            if n > 129:
                continue
            fd = vm.central_x(lambda v: float(np.dot(c, prox(v))), x.copy())
            worst = max(worst, float(np.max(np.abs(fd - gx))))
            assert np.max(np.abs(fd - gx)) <= vm.FD_TOL, (n, lam, weighted)
            if n < 2:
                continue
            if not weighted:
                dl = (np.dot(c, oracle.tv1_hybrid(x, lam + vm.FD_H)) - np.dot(c, oracle.tv1_hybrid(x, lam - vm.FD_H))) / (2 * vm.FD_H)
                worst = max(worst, abs(dl - gw.sum()))
                assert abs(dl - gw.sum()) <= vm.FD_TOL, (n, lam)
            elif n <= 65:
                fdw = vm.central_x(lambda ww: float(np.dot(c, oracle.tv1_weighted(x, ww))), w.copy())
                worst = max(worst, float(np.max(np.abs(fdw - gw))))
                assert np.max(np.abs(fdw - gw)) <= vm.FD_TOL, (n, lam)
    print(f"closed form vs central differences: worst {worst:.3e} (bar {vm.FD_TOL:.0e})")


def test_model_constants_are_the_headers():
    """tests/vjp_model.py restates the step rule; the numbers must be the ones the public header documents."""
    text = open(os.path.join(HERE, "..", "include", "proxtv_amd.h")).read()
    m = re.search(r"STEP iff \|y\[k\+1\] - y\[k\]\| > (\d+) \* 2\^-52 \* max\(\|y\[k\]\|, \|y\[k\+1\]\|\) \+ ([0-9.e-]+) ", text)
    assert m, "the header no longer states the step rule"
    assert float(m.group(1)) * 2.0 ** -52 == vm.STEP_REL and float(m.group(2)) == vm.STEP_ABS


# ---- (b) the host build of vjpcore.hpp ---------------------------------------------------------------------------------------------
def test_step_rule_is_the_certifiers(harness):
    rule = np.zeros(2)
    harness.vjp_host_step_rule(rule.ctypes.data)
    assert rule[0] == vm.STEP_REL and rule[1] == vm.STEP_ABS
    for a, b in ((0.0, 4e-10), (0.0, 4.0000001e-10), (1.0, 1.0 + 4e-10 + 256 * 2.0 ** -52), (1.0, 1.0 + 5e-10), (-3.0, -3.0), (1e9, 1e9 + 1e-4),
                 (1e9, 1e9 - 1e-3), (2.0, -2.0)):
        assert bool(harness.vjp_host_is_step(a, b)) == bool(vm.steps(np.array([a, b]))[0]), (a, b)


def fibres(oracle):
    """(name, y, g): the prox of every case of (a), uniform and weighted, plus an all-equal fibre, a strictly monotone one and one whose
    steps sit exactly at the boundaries of chunks of 1, 2, 7 and 64 samples."""
    for n, lam, x, c, w in vm.cases():
        yield f"n{n} lam{lam}", oracle.tv1_hybrid(x, lam), c
        if n >= 2:
            yield f"n{n} lam{lam} weighted", oracle.tv1_weighted(x, w), c
    rng = np.random.default_rng(7)
    yield "all equal", np.full(200, 0.75), rng.standard_normal(200)
    yield "strictly monotone", np.cumsum(rng.uniform(0.1, 1.0, 200)), rng.standard_normal(200)
    yield "monotone down", -np.cumsum(rng.uniform(0.1, 1.0, 131)), rng.standard_normal(131)
    levels = np.repeat(rng.standard_normal(6), 2 * 7 * 64)[:5 * 896 + 300]      # steps at multiples of 896 = lcm(1, 2, 7, 64) * 2
    yield "steps at chunk boundaries", levels, rng.standard_normal(levels.size)


def test_chunked_phases_equal_the_model(harness, oracle):
    """Phases A, B, C through vjpcore.hpp for chunks of 1, 2, 7 and 64 samples: gx within 64 n 2^-52 max|g| of the numpy model (the
    certifier's rounding rule), gw within twice that, the segment count exact; in place (gx is g) gives the same bits; a segment has one
    value, bit for bit, however many chunks it spans."""
    for name, y, g in fibres(oracle):
        vm.assert_unambiguous(y)
        n = y.size
        want_gx, want_gw, want_nseg = vm.vjp_1d(y, g)
        bound = vm.rounding_bound(n, g)
        for chunk in CHUNKS:
            gx, gw, nseg = run(harness, y, g, chunk)
            assert nseg == want_nseg, (name, chunk)
            assert np.max(np.abs(gx - want_gx)) <= bound, (name, chunk)
            if n > 1:
                assert np.max(np.abs(gw - want_gw)) <= 2 * bound, (name, chunk)
                assert np.all(gw[~vm.steps(y)] == 0.0), (name, chunk)
                assert np.all(np.diff(gx)[~vm.steps(y)] == 0.0), (name, chunk)
            gx2, gw2, _ = run(harness, y, g, chunk, inplace=True)
            assert np.array_equal(gx2, gx) and np.array_equal(gw2, gw), (name, chunk)
            gx3, _, nseg3 = run(harness, y, g, chunk, want_gw=False)
            assert np.array_equal(gx3, gx) and nseg3 == nseg, (name, chunk)


def test_degenerate_penalties_on_the_host(harness, oracle):
    """lambda = 0: the prox is the identity, every sample its own segment, gx = g exactly.  A penalty that flattens the fibre: gx is the
    mean of g, gw = 0."""
    rng = np.random.default_rng(11)
    x, g = rng.standard_normal(150), rng.standard_normal(150)
    for chunk in CHUNKS:
        gx, gw, nseg = run(harness, x, g, chunk)
        assert np.array_equal(gx, g) and nseg == 150
        flat = oracle.tv1_hybrid(x, 1e6)
        vm.assert_unambiguous(flat)
        gx, gw, nseg = run(harness, flat, g, chunk)
        assert nseg == 1 and np.all(gw == 0.0) and np.all(gx == gx[0]) and abs(gx[0] - g.mean()) <= vm.rounding_bound(150, g)
