"""The derivative of the general-p TV-Lp fibre prox without a GPU: (1) the dense model (tests/tvp_fibres_vjp_model.py)
against central differences of the host-built forward (tvpcore.hpp), (2) the per-fibre functions the HIP kernel runs
(proxtv_amd/csrc/tvpvjpcore.hpp), compiled for the host by tests/tvp_vjp_host.cpp, against that model, (3) the symmetry of the Jacobian,
(4) the closed forms, (5) the limit p -> 2 against the TV-L2 model."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import tv2_vjp_model as t2
import tvp_fibres_vjp_model as tm

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def host():
    out = os.path.join(tempfile.mkdtemp(prefix="ptv_tvp_vjp_"), "libtvp_vjp_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "tvp_vjp_host.cpp")],
                   check=True)
    lib = C.CDLL(out)
    lib.host_tvp_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    lib.host_tvp_forward.restype = C.c_int
    lib.host_tvp_vjp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int]
    lib.host_tvp_vjp.restype = C.c_double
    return lib


def forward(lib, y, lam, p):
    """(x, iterative): the host-built prox and whether the forward iterated (False: a closed form -- a copy or the mean)."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    x, outer = np.full(y.size, np.nan), C.c_int()
    capped = lib.host_tvp_forward(y.ctypes.data, x.ctypes.data, y.size, float(lam), float(p), None, C.byref(outer))
    assert not capped
    return x, outer.value > 0


def core(lib, x, g, lam, p, inc=1, inplace=False):
    x = np.ascontiguousarray(x, dtype=np.float64)
    g = np.array(g, dtype=np.float64)
    gx = g if inplace else np.full(x.size, np.nan)
    glam = lib.host_tvp_vjp(x.ctypes.data, g.ctypes.data, gx.ctypes.data, x.size, float(lam), float(p), inc)
    return gx, glam


@pytest.fixture(scope="module")
def solved(host):
    """Every case of the grid with its forward output, computed once: (n, p, lam, y, g, o, x, iterative)."""
    return [(n, p, lam, y, g, o) + forward(host, y, lam, p) for n, p, lam, y, g, o in tm.cases()]


# ---- (1) the model against central differences of the forward -----------------------------------------------------------------------
def test_model_equals_central_differences_of_the_forward(host, solved):
    """gx (through the whole Jacobian, column by column: no symmetry assumed) and glam against central differences with h = 1e-5 of the
    host-built forward, per arm within tm.FD_BAR -- four times the largest difference measured on this grid (dual 6.3e-6, primal 8.7e-5;
    the forward stops at a duality gap of 1e-8 and the derivative of what it leaves is what the differences see).  A case is left out
    only where a +-h perturbation changes the forward's branch (iterative against mean); at most a tenth of the grid."""
    h = tm.FD_H
    worst, left_out = {"dual": 0.0, "primal": 0.0}, 0
    for n, p, lam, y, g, o, x, iterative in solved:
        gx, glam = tm.vjp_1d(x, g, lam, p)
        jac, same = np.empty((n, n)), True
        for j in range(n):
            e = np.zeros(n)
            e[j] = h
            (xp, ip), (xm, im) = forward(host, y + e, lam, p), forward(host, y - e, lam, p)
            same = same and ip == iterative and im == iterative
            jac[:, j] = (xp - xm) / (2 * h)
        (xp, ip), (xm, im) = forward(host, y, lam + h, p), forward(host, y, lam - h, p)
        same = same and ip == iterative and im == iterative
        if not same:
            left_out += 1
            continue
        ex = float(np.max(np.abs(jac.T @ g - gx)))
        el = abs(float(g @ (xp - xm)) / (2 * h) - glam)
        if max(ex, el) > 0.5 * worst[tm.arm(p)]:
            print(f"n {n} p {p} lambda {lam}: |gx - fd| {ex:.2e}, |glam - fd| {el:.2e}")
        worst[tm.arm(p)] = max(worst[tm.arm(p)], ex, el)
        assert ex <= tm.FD_BAR[tm.arm(p)] and el <= tm.FD_BAR[tm.arm(p)], (n, p, lam, ex, el)
    print(f"model vs central differences: worst {worst}, bars {tm.FD_BAR}, {left_out} of {len(solved)} left out")
    assert 10 * left_out <= len(solved)


# ---- (2) the host build of tvpvjpcore.hpp against the model -------------------------------------------------------------------------
def test_host_core_equals_the_model(host, solved):
    """tvpvjpcore.hpp on the forward's output: gx and glam within tm.bar of the dense model -- 64 n ulps of max|g|, times the condition
    number of the arm's matrix, times 1 / (1 - c b'e) (p > 2) or ||w||^2 / (w'e) (p < 2); a strided layout and in place (gx is g) give
    the same bits; both arms, the mean and the copy occur."""
    worst, kinds = 0.0, set()
    for n, p, lam, y, g, o, x, iterative in solved:
        want_gx, want_glam = tm.vjp_1d(x, g, lam, p)
        bound = tm.bar(x, g, lam, p)
        gx, glam = core(host, x, g, lam, p)
        ex, el = float(np.max(np.abs(gx - want_gx))), abs(glam - want_glam)
        worst = max(worst, ex / bound, el / bound)
        assert ex <= bound and el <= bound, (n, p, lam, ex, el, bound)
        kinds.add((tm.arm(p) if iterative else "closed"))
        if not iterative:
            assert glam == 0.0 and np.all(gx == gx[0]), (n, p, lam)
        for inc, inplace in ((3, False), (1, True), (5, True)):
            gx2, glam2 = core(host, x, g, lam, p, inc, inplace)
            assert np.array_equal(gx2, gx) and glam2 == glam, (n, p, lam, inc, inplace)
    print(f"host core vs model: worst ratio to the bar {worst:.2e}")
    assert kinds == {"dual", "primal", "closed"}


# ---- (3) symmetry ----------------------------------------------------------------------------------------------------------------------
def test_the_jacobian_is_symmetric(host, solved):
    """o'(J g) == g'(J o) through the host core, within the rounding of the two products at the bar of (2)."""
    for n, p, lam, y, g, o, x, iterative in solved:
        jg, _ = core(host, x, g, lam, p)
        jo, _ = core(host, x, o, lam, p)
        sym = n * (float(np.max(np.abs(o))) * tm.bar(x, g, lam, p) + float(np.max(np.abs(g))) * tm.bar(x, o, lam, p))
        assert abs(float(o @ jg) - float(g @ jo)) <= sym, (n, p, lam)


# ---- (4) closed forms ------------------------------------------------------------------------------------------------------------------
def test_closed_forms(host):
    """n = 1 and lambda = 0: gx = g bit for bit; a constant output: gx = mean(g), also at lambda = 1e6; glam exactly 0 in all of them --
    in the model and in the host core."""
    rng = np.random.default_rng(5)
    for p in tm.PS:
        for n in (1, 2, 9, 17):
            x, g = rng.standard_normal(n), rng.standard_normal(n)
            for lam in ((0.5, 0.0, 1e6) if n == 1 else (0.0,)):
                for gx, glam in (tm.vjp_1d(x, g, lam, p), core(host, x, g, lam, p), core(host, x, g, lam, p, 2, True)):
                    assert np.array_equal(gx, g) and glam == 0.0, (p, n, lam)
            if n > 1:
                const = np.full(n, 0.3)
                for lam in (0.5, 1e6):
                    for gx, glam in (tm.vjp_1d(const, g, lam, p), core(host, const, g, lam, p), core(host, const, g, lam, p, 2, True)):
                        assert glam == 0.0 and np.all(gx == gx[0]) and abs(gx[0] - g.mean()) <= 4 * n * 2.0 ** -52 * np.abs(g).max()
                # and through the forward: a penalty this large answers with the mean itself
                xf, iterative = forward(host, x, 1e6, p)
                assert not iterative and np.all(xf == xf[0])
                gx, glam = core(host, xf, g, 1e6, p)
                assert glam == 0.0 and np.all(gx == gx[0]) and abs(gx[0] - g.mean()) <= 4 * n * 2.0 ** -52 * np.abs(g).max()


# ---- (5) the limit p -> 2 --------------------------------------------------------------------------------------------------------------
def test_both_arms_approach_the_tv_l2_derivative(host):
    """At p = 2 -+ 1e-3 the model lies within 1e-2 max|g| of the TV-L2 model on the same output, on cases clear of the TV-L2 kink (a
    sanity check of both arms, not a precision claim)."""
    rng = np.random.default_rng(9)
    checked = 0
    for n in (3, 9, 17, 64):
        for lam in (0.05, 0.8, 3.0):
            y, g = rng.standard_normal(n), rng.standard_normal(n)
            un = t2.dual_norm(y)
            if un <= lam * (1 + t2.KINK_CLEAR):      # (inside the ball or near it: the TV-L2 prox is the mean there)
                continue
            for p in (2.0 - 1e-3, 2.0 + 1e-3):
                x, iterative = forward(host, y, lam, p)
                assert iterative
                mu = float(np.linalg.norm(np.diff(x))) / lam
                want_gx, want_glam = t2.vjp_1d(x, mu, g, lam)
                gx, glam = tm.vjp_1d(x, g, lam, p)
                tol = 1e-2 * float(np.max(np.abs(g)))
                assert float(np.max(np.abs(gx - want_gx))) <= tol and abs(glam - want_glam) <= tol, (n, lam, p)
                checked += 1
    assert checked >= 12
