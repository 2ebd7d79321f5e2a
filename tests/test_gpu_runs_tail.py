"""Known runs on the segment that holds the fibre's last sample (sweep_along_kernel RUNS under `endseg`; chunkcore.hpp free_end_edges /
free_end_settle) on the GPU: the fibre's end is a free end like its start, so the end segment of a dimension-0 sweep on rung 0 is cut at
its known bends and solved run by run like the interior ones, and falls back to the speculative walk where it does not fit.

Columns through tvgen against the CPU oracle's fibre prox, against the same call with option "runs" off, twice for bit-reproducibility,
with the "why" counter of waves solved run by run counting the end segments too; the families that stress the free end; small DR
solves; and the places it stays out of.

Engagement on the noise columns below, measured beforehand on the host with tests/runs_tail_harness.cpp (tests/test_runs_tail_host.py,
test_engagement_on_the_gpu_tests_columns, the same seed and shapes): 7 of 448 end segments fall back (1.6 %), all for want of a known
bend within two samples of the segment's start; the bar here, for interior and end segments together, is 10 %."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import assert_close

pytestmark = pytest.mark.gpu

ROWS, SEED = (1110, 2177, 3281, 4080, 4081, 4096, 4097), 191     # (tests/test_runs_tail_host.py draws the same columns)


@pytest.fixture()
def why(clib):
    before = (clib.proxtv_set_option(b"why", 1), clib.proxtv_set_option(b"chunk_mode", -1))
    if before[1] != -1:
        clib.proxtv_set_option(b"why", before[0])
        clib.proxtv_set_option(b"chunk_mode", before[1])
        pytest.skip("a pinned rung (PROXTV_CHUNK_MODE): the seeded policy decides where runs are used")
    buf = (C.c_uint * 8)()

    def read():
        clib.proxtv_debug_why(buf)
        return np.array(list(buf), dtype=np.int64)
    read()
    yield read
    clib.proxtv_set_option(b"why", before[0])


@functools.lru_cache(maxsize=None)
def noise():
    rng = np.random.default_rng(SEED)
    return {M: rng.standard_normal((M, 64)) for M in ROWS}


def _columns(ptv, X, lam):
    return ptv.tvgen(X, [lam], [1], [1])


def _oracle_columns(oracle, X, lam):
    return np.apply_along_axis(lambda f: oracle.tv1_hybrid(np.ascontiguousarray(f), lam), 0, X)


def _without_runs(ptv, clib, X, lam, why):
    before = clib.proxtv_set_option(b"runs", 0)
    try:
        why()
        plain = _columns(ptv, X, lam)
        assert why()[5] == 0
    finally:
        clib.proxtv_set_option(b"runs", before)
    return plain


@pytest.mark.parametrize("M", ROWS)
def test_noisy_columns_end_segment_included(ptv, clib, oracle, why, M):
    X = noise()[M]
    why()
    got = _columns(ptv, X, 0.1)
    w = why()
    assert_close(got, _oracle_columns(oracle, X, 0.1), tol=1e-12, what=f"columns {M} x 64")
    interior = (M - 9) // 1088          # segments whose window and look-ahead lie inside the fibre; + 1: the one with the last sample
    assert w[5] >= 0.9 * (interior + 1) * 64, (w, interior)
    assert_close(got, _without_runs(ptv, clib, X, 0.1, why), tol=1e-13, what=f"columns {M} x 64, against the speculative path")
    assert np.array_equal(got, _columns(ptv, X, 0.1)), "two calls differ"


def tail_families(M, seed):
    """(name, M x 64 image, penalty): what the free end has to survive, one variant a column."""
    rng = np.random.default_rng(seed)
    lam = 0.1
    X = rng.standard_normal((M, 64))
    for c in range(64):        # last runs of 1, 2, 3, 14 and 15 samples behind a jump of 30 lambda (15: longer than a lane takes)
        run = (1, 2, 3, 14, 15)[c % 5]
        X[M - run:, c] = X[M - run - 1, c] + 30.0 * lam + 0.01 * rng.standard_normal(run)
    yield "short last runs", X, lam
    X = rng.standard_normal((M, 64))
    X[-40:] = X[-40]
    yield "constant tail", X, lam
    yield "integer ties", rng.integers(-2, 3, (M, 64)).astype(float), 0.25
    # jumps of exactly 0, 2 lambda, 4 lambda and 4 lambda (1 +- 6e-9) on the fibre's last two edges behind a known bend of either type
    # (lambda = 1/4 on multiples of 2^-12: "exactly" to the last bit)
    lam = 0.25
    X = np.round(rng.standard_normal((M, 64)) * 2.0 * 4096.0) / 4096.0
    jumps = np.array([0.0, 2.0, 4.0, 4.0 * (1 + 6e-9), 4.0 * (1 - 6e-9)])
    X[-3] = X[-4] + rng.choice([-1.0, 1.0], 64) * np.round((5.0 + rng.random(64)) * lam * 4096.0) / 4096.0
    X[-2] = X[-3] + rng.choice([-1.0, 1.0], 64) * jumps[np.arange(64) % 5] * lam
    X[-1] = X[-2] + rng.choice([-1.0, 1.0], 64) * jumps[(np.arange(64) // 5) % 5] * lam
    yield "slivers at the fibre's end", X, lam


@pytest.mark.parametrize("M", (4096, 2177))
def test_tail_families(ptv, clib, oracle, why, M):
    c0 = clib.proxtv_debug_counter(b"certify_failures")
    for name, X, lam in tail_families(M, 1000 + M):
        certify = name.startswith("slivers")
        if certify:
            clib.proxtv_set_option(b"certify", 1)
        try:
            why()
            got = _columns(ptv, X, lam)
            w = why()
        finally:
            if certify:
                clib.proxtv_set_option(b"certify", 0)
        assert_close(got, _oracle_columns(oracle, X, lam), tol=1e-12, what=f"{M} x 64, {name}")
        assert_close(got, _without_runs(ptv, clib, X, lam, why), tol=1e-13, what=f"{M} x 64, {name}, against the speculative path")
        if name == "constant tail":      # (no bend in reach of the end: every end segment falls back, the interior ones do not care)
            segments = (M - 9) // 1088 + 1          # per fibre: the interior ones and the one with the last sample
            assert w[6] * segments >= w[5] + w[6] > 0, (name, w)     # (counted per wave, however many sweeps the call took)
    assert clib.proxtv_debug_counter(b"certify_failures") == c0


@pytest.mark.parametrize("M", (4096, 2177))
def test_dr_solves(ptv, oracle, M):
    X = np.random.default_rng(M + 7).standard_normal((M, 8))
    got = ptv.tv1_2d(X, 0.1)
    assert_close(got, oracle.dr2(X, 0.1)[0], tol=1e-9, what=f"dr2 {M} x 8")
    assert np.array_equal(got, ptv.tv1_2d(X, 0.1))


def test_it_stays_out_of_one_segment_fibres_and_weighted_sweeps(ptv, clib, why):
    rng = np.random.default_rng(192)
    X = rng.standard_normal((2300, 64))
    why()
    _columns(ptv, X[:1000], 0.1)
    ptv.tv1w_2d(X, rng.uniform(0.05, 0.15, (2299, 64)), rng.uniform(0.05, 0.15, (2300, 63)), max_iters=2)
    assert why()[5] == 0
