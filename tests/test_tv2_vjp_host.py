"""The derivative of the 1-D TV-L2 prox without a GPU: (a) the closed form (tests/tv2_vjp_model.py) against central differences of the
CPU oracle, (b) the per-fibre functions the HIP kernel runs (proxtv_amd/csrc/tv2vjpcore.hpp), compiled for the host by
tests/tv2_vjp_host.cpp, against that model."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import tv2_vjp_model as tm
import vjp_model as vm

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(tempfile.mkdtemp(prefix="ptv_tv2_vjp_"), "libtv2_vjp_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "tv2_vjp_host.cpp")],
                   check=True)
    lib = C.CDLL(out)
    lib.tv2_vjp_host_run.restype = C.c_double
    lib.tv2_vjp_host_run.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.c_double, C.c_void_p]
    lib.tv2_vjp_host_kfix.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_int]
    return lib


def run(lib, y, mu, g, lam, inplace=False):
    y = np.ascontiguousarray(y, dtype=np.float64)
    g = np.array(g, dtype=np.float64)
    gx = g if inplace else np.full(y.size, np.nan)
    glam = lib.tv2_vjp_host_run(y.ctypes.data, float(mu), g.ctypes.data, y.size, float(lam), gx.ctypes.data)
    return gx, glam


def prox(oracle, x, lam):
    return oracle.tv(x, lam, 2)[0]


# ---- (a) the closed form against the oracle ----------------------------------------------------------------------------------------
def test_closed_form_equals_central_differences_of_the_oracle(oracle):
    """gx and glam against central differences (h = 1e-5) of c . prox with the oracle's exact TV-L2 prox: within 1e-8.  A case within 5 %
    of the kink is skipped (the differences straddle it), at most 1 in 10; every case checks the symmetry of the Jacobian and what the
    inside case and the degenerate ones must give."""
    worst, skipped, total = 0.0, 0, 0
    for n, lam, x, c, o in tm.cases():
        total += 1
        y = prox(oracle, x, lam)
        mu, un = tm.mu_of(x, y, lam)
        gx, glam = tm.vjp_1d(y, mu, c, lam)
        gxo, _ = tm.vjp_1d(y, mu, o, lam)
        # o' J c == c' J o within the rounding of the two products
        sym = n * (float(np.max(np.abs(o))) * tm.bar(n, mu, c) + float(np.max(np.abs(c))) * tm.bar(n, mu, o))
        assert abs(np.dot(o, gx) - np.dot(c, gxo)) <= sym, (n, lam)
        if n == 1:
            assert np.array_equal(gx, c) and glam == 0.0
        elif mu == 0.0:
            assert glam == 0.0 and np.all(gx == gx[0]) and abs(gx[0] - c.mean()) <= vm.rounding_bound(n, c), (n, lam)
        if n > 1 and tm.near_kink(un, lam):
            skipped += 1
            continue
        assert n == 1 or abs(un - lam) >= tm.KINK_CLEAR * lam, (n, lam, un)      # (a property of the inputs: see tm.SEED)
        fd = vm.central_x(lambda v: float(np.dot(c, prox(oracle, v, lam))), x.copy())
        ex = float(np.max(np.abs(fd - gx)))
        dl = (np.dot(c, prox(oracle, x, lam + vm.FD_H)) - np.dot(c, prox(oracle, x, lam - vm.FD_H))) / (2 * vm.FD_H)
        el = abs(dl - glam)
        print(f"n {n} lambda {lam}: mu {mu:.3e}, |gx - fd| {ex:.2e}, |glam - fd| {el:.2e}")
        worst = max(worst, ex, el)
        assert ex <= vm.FD_TOL and el <= vm.FD_TOL, (n, lam, mu)
    print(f"closed form vs central differences: worst {worst:.3e} (bar {vm.FD_TOL:.0e}), {skipped} of {total} skipped")
    assert 10 * skipped <= total


def test_both_branches_occur(oracle):
    """The cases hold inside fibres and active ones, and lambda = 0 is the identity."""
    mus = [tm.mu_of(x, prox(oracle, x, lam), lam)[0] for n, lam, x, c, o in tm.cases() if n > 1]
    assert any(m == 0.0 for m in mus) and any(m > 0.0 for m in mus)
    rng = np.random.default_rng(3)
    x, c = rng.standard_normal(20), rng.standard_normal(20)
    gx, glam = tm.vjp_1d(x, 0.0, c, 0.0)
    assert np.array_equal(gx, c) and glam == 0.0


# ---- (b) the host build of tv2vjpcore.hpp ------------------------------------------------------------------------------------------
def fibres(oracle):
    """(name, n, lambda, y, mu, g): every case of (a), then n = 300 and n = 1000 at penalties that keep the multiplier above 1e-3."""
    for n, lam, x, c, o in tm.cases():
        y = prox(oracle, x, lam)
        yield f"n{n} lam{lam}", n, lam, y, tm.mu_of(x, y, lam)[0], c
    rng = np.random.default_rng(17)
    for n in (300, 1000):
        for lam in (0.8, 3.0, 12.0):
            x, c = rng.standard_normal(n), rng.standard_normal(n)
            y = prox(oracle, x, lam)
            mu = tm.mu_of(x, y, lam, banded=True)[0]
            assert mu >= 1e-3, (n, lam, mu)
            yield f"n{n} lam{lam}", n, lam, y, mu, c


def test_host_build_equals_the_model(harness, oracle):
    """eliminate + substitute through tv2vjpcore.hpp: gx within 64 n 2^-52 cond(M) max|g| of the dense model, cond(M) = (4 + mu) /
    (mu + 4 sin^2(pi / 2n)), and glam within the same bound; in place (gx is g) gives the same bits."""
    worst = 0.0
    for name, n, lam, y, mu, g in fibres(oracle):
        want_gx, want_glam = tm.vjp_1d(y, mu, g, lam)
        bound = tm.bar(n, mu, g)
        gx, glam = run(harness, y, mu, g, lam)
        ex = float(np.max(np.abs(gx - want_gx)))
        el = abs(glam - want_glam)
        worst = max(worst, ex / bound, el / bound)
        print(f"{name}: mu {mu:.3e}, |gx - model| {ex:.2e}, |glam - model| {el:.2e}, bound {bound:.2e}")
        assert ex <= bound, name
        assert el <= bound, name
        if n == 1:
            assert np.array_equal(gx, g) and glam == 0.0
        elif mu == 0.0:
            assert glam == 0.0 and np.all(gx == gx[0]), name
        gx2, glam2 = run(harness, y, mu, g, lam, inplace=True)
        assert np.array_equal(gx2, gx) and glam2 == glam, name
    print(f"host build vs model: worst ratio to the bar {worst:.2e}")


def test_pivots_reach_their_fixed_point(harness, oracle):
    """With mu ~ 1 the reciprocal pivots stop changing after a few dozen edges and are no longer stored (kfix < n - 1); with mu = 0
    (pivots (i + 2) / (i + 1)) they never do.  Either way the result is the model's (the test above); here: the switch is exercised."""
    rng = np.random.default_rng(23)
    n = 300
    x, c = rng.standard_normal(n), rng.standard_normal(n)
    y = prox(oracle, x, 0.8)
    mu = tm.mu_of(x, y, 0.8)[0]
    assert mu > 0.1
    y = np.ascontiguousarray(y)
    kfix = harness.tv2_vjp_host_kfix(y.ctypes.data, mu, c.ctypes.data, n)
    assert 1 <= kfix < 100, kfix
    assert harness.tv2_vjp_host_kfix(y.ctypes.data, 0.0, c.ctypes.data, n) == n - 1


def test_degenerate_penalties_on_the_host(harness):
    """lambda = 0 and n = 1: gx = g exactly, glam = 0, whatever mu says."""
    rng = np.random.default_rng(11)
    for n in (1, 2, 150):
        x, g = rng.standard_normal(n), rng.standard_normal(n)
        for mu, lam in ((0.0, 0.0), (0.7, 0.0), (0.0, -1.0)) + (((0.7, 1.0),) if n == 1 else ()):
            gx, glam = run(harness, x, mu, g, lam)
            assert np.array_equal(gx, g) and glam == 0.0, (n, mu, lam)
