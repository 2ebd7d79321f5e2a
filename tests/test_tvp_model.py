"""The yardstick of the general-p tests (tests/tvp_model.py) against what is already trusted -- no GPU needed: on the reference's own
outputs (tests/golden/golden_pgen.npz) tvp_gap is within the reference's stopping rule, and at p = 2 it is test_oracle_p2's kkt_gap."""
import numpy as np
import pytest

import tvp_model as tm
from conftest import load_golden
from test_oracle_p2 import kkt_gap


@pytest.fixture(scope="module")
def gpg():
    return load_golden("golden_pgen.npz")


def test_the_golden_grid_is_the_models(gpg):
    assert np.array_equal(gpg["grid"], np.array(tm.GRID, dtype=np.float64))
    assert len(tm.GRID) == 5 * 4 * 3 - 1 + 5 * 2
    for n in (2, 3, 17, 100, 1000):
        assert np.array_equal(gpg[f"y_{n}"], tm.signal(n, int(gpg["seed"])))


def test_tvp_gap_of_the_reference_outputs_is_within_its_stopping_rule(gpg):
    worst = 0.0
    for k, (n, p, lam) in enumerate(tm.GRID):
        y, x, info = gpg[f"y_{n}"], gpg[f"x_{k}"], gpg[f"info_{k}"]
        gap = tm.tvp_gap(x, y, lam, p)
        worst = max(worst, gap)
        assert info[2] == 0, (n, p, lam)
        assert -1e-12 * max(1.0, tm.primal(x, y, lam, p)) <= gap <= 1e-5, (n, p, lam, gap)
    print(f"largest tvp_gap of a reference output: {worst:.3e}")


def test_tvp_gap_is_kkt_gap_at_p_2():
    rng = np.random.default_rng(3)
    for n in (2, 3, 17, 100):
        y = tm.signal(n, 5)
        for lam in (0.05, 1.0, 30.0):
            for x in (y + 0.1 * rng.standard_normal(n), np.full(n, y.mean()), y.copy()):
                a, b = tm.tvp_gap(x, y, lam, 2.0), kkt_gap(x, y, lam)[0]
                assert abs(a - b) <= 1e-12 * max(1.0, abs(b)), (n, lam, a, b)


def test_tvp_gap_bounds_the_distance_to_the_minimiser():
    """1-strong convexity: ||x - x*||^2 <= 2 (P(x) - P*) <= 2 tvp_gap(x); x* from the golden (itself within sqrt(2e-5) of the minimiser)."""
    gpg = load_golden("golden_pgen.npz")
    rng = np.random.default_rng(4)
    for k, (n, p, lam) in enumerate(tm.GRID):
        if n not in (17, 100):
            continue
        y, xs = gpg[f"y_{n}"], gpg[f"x_{k}"]
        x = xs + 0.05 * rng.standard_normal(n)
        assert np.linalg.norm(x - xs) <= tm.radius(x, y, lam, p) + np.sqrt(2e-5), (n, p, lam)


def test_lp_norm():
    v = np.array([3.0, -4.0, 0.0])
    assert tm.lp_norm(v, 2) == pytest.approx(5.0, rel=1e-15)
    assert tm.lp_norm(v, 1) == pytest.approx(7.0, rel=1e-15)
    assert tm.lp_norm(v, np.inf) == 4.0
    assert tm.lp_norm(1e200 * v, 50) == pytest.approx(1e200 * np.sum(np.abs(v) ** 50.0) ** 0.02, rel=1e-13)
    assert tm.lp_norm(np.zeros(4), 3) == 0.0 and tm.lp_norm([], 3) == 0.0
