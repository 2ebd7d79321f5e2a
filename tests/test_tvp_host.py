"""The general-p TV-Lp fibre solver (proxtv_amd/csrc/tvpcore.hpp: nested Newton iterations on the dual's KKT system), compiled for the
host, one fibre per call -- no GPU needed.  The bars are the GPU test's: the model's duality gap of the output within 1e-5, the solver's
own figure equal to it, the mean kept, no cap hit, and the reference's output within what the two gaps allow."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import tvp_model as tm
from conftest import load_golden

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def solve():
    out = os.path.join(tempfile.mkdtemp(prefix="ptv_tvp_"), "libtvp_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "tvp_host.cpp")],
                   check=True)
    lib = C.CDLL(out)
    lib.host_tvp_fibre.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.host_tvp_fibre.restype = C.c_int

    def run(y, lam, p):
        y = np.ascontiguousarray(y, dtype=np.float64)
        x, gap, outer, sweeps = np.full(y.size, np.nan), C.c_double(), C.c_int(), C.c_int()
        capped = lib.host_tvp_fibre(y.ctypes.data, x.ctypes.data, y.size, lam, p, C.byref(gap), C.byref(outer), C.byref(sweeps))
        return x, gap.value, outer.value, sweeps.value, capped
    return run


def test_golden_grid(solve):
    gpg = load_golden("golden_pgen.npz")
    most = 0
    for k, (n, p, lam) in enumerate(tm.GRID):
        y, ref = gpg[f"y_{n}"], gpg[f"x_{k}"]
        x, gap, outer, sweeps, capped = solve(y, lam, p)
        scale, pmean = max(1.0, np.abs(y).max()), tm.primal(np.full(n, y.mean()), y, lam, p)
        model = tm.tvp_gap(x, y, lam, p)
        most = max(most, sweeps)
        assert not capped and model <= 1e-5, (n, p, lam, model)
        assert abs(x.mean() - y.mean()) <= 1e-12 * scale
        assert abs(gap - model) <= 0.1 * model + 1e-10 * max(1.0, pmean), (n, p, lam, gap, model)
        assert np.linalg.norm(x - ref) <= tm.radius(x, y, lam, p) + tm.radius(ref, y, lam, p) + 1e-12 * scale
    print("most forward sweeps of a case:", most)
    assert most <= 200     # (the cap is 1500)


def test_closed_forms(solve):
    y = tm.signal(17, 2)
    for p in (1.5, 3.0):
        x, gap, outer, _, capped = solve(y[:1], 1.0, p)
        assert np.array_equal(x, y[:1]) and gap == 0 and outer == 0 and not capped
        x, gap, outer, _, capped = solve(y, 0.0, p)
        assert np.array_equal(x, y) and gap == 0 and outer == 0
        x, gap, outer, _, capped = solve(y, 1e6, p)
        assert np.abs(x - y.mean()).max() <= 1e-12 * np.abs(y).max() and gap == 0 and outer == 0
        x, gap, outer, _, capped = solve(np.full(9, 0.3), 0.5, p)
        assert np.array_equal(x, np.full(9, 0.3)) and outer == 0


def test_the_ends_of_the_accepted_range_come_back_feasible(solve):
    """Exponents up to 500 on either side: whatever the caps do, the output keeps the mean and its reported gap is the model's."""
    for p in (1.0021, 1.01, 1.9, 2.1, 50.0, 99.9):
        for n, lam in ((17, 0.05), (100, 1.0), (100, 30.0)):
            y = tm.signal(n, 7)
            x, gap, outer, sweeps, capped = solve(y, lam, p)
            model = tm.tvp_gap(x, y, lam, p)
            pmean = tm.primal(np.full(n, y.mean()), y, lam, p)
            assert np.all(np.isfinite(x)) and sweeps <= 1500 + 100
            assert abs(x.mean() - y.mean()) <= 1e-12 * np.abs(y).max()
            assert abs(gap - model) <= 0.1 * model + 1e-10 * max(1.0, pmean), (p, n, lam, gap, model)
            assert capped or model <= 1e-5
