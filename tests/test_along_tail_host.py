"""The along-fibre kernel's segment with the fibre's last sample, on the host (tests/along_tail_harness.cpp): it is staged with rows past
the last sample clamped to it and rebuilt with the register-resident form that takes a row count per lane (chunkcore.hpp rebuild_owned,
FULL = 3) instead of the general form.

What is checked: for fibre lengths at which the end segment takes every shape the kernel distinguishes -- one sample, less than a chunk,
whole chunks only, a partial last chunk, a full segment -- the new form leaves the bits of the general form in every row of the window
and writes the same rows (none outside the segment, none past the fibre), for an op that uses the row's own sample and one that does not;
and where the segment's links hold, the rows are the prox.  Twice, like the chunk tests: IEEE quotients and the device's table
reciprocals."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# C = 17, SEG = 1088: an end segment of one sample; around the edge of `interior` (seg_s + SEG + T <= len - 1); one whole chunk; a whole
# chunk and a partial one; ending on a segment, and one more; a whole-chunk boundary; around the chunk boundary next to 4096's partial last
# chunk; the workload's shape, and one more; four full segments; five segments
LENGTHS = (1089, 1096, 1097, 1098, 1105, 1110, 2176, 2177, 3264 + 17, 4079, 4080, 4081, 4096, 4097, 4352, 5000)


@pytest.fixture(scope="module", params=["quotients", "table reciprocals"])
def harness(request):
    out = os.path.join(tempfile.mkdtemp(prefix="ptv_tail_"), "libalong_tail.so")
    flags = ["-DPTV_TABLE_RECIP"] if request.param == "table reciprocals" else []
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", *flags, "-o", out,
                    os.path.join(HERE, "along_tail_harness.cpp")], check=True)
    lib = C.CDLL(out)
    lib.host_tail_rebuild.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def rebuild(lib, y, lam, reflect):
    y = np.ascontiguousarray(y, dtype=np.float64)
    x = np.full(y.size, np.nan)
    stats = np.zeros(6, dtype=np.int32)
    rc = lib.host_tail_rebuild(y.ctypes.data, lam, y.size, int(reflect), x.ctypes.data, stats.ctypes.data)
    assert rc == 0, f"the two rebuild forms differ in {-rc} rows / write counts (len {y.size}, lambda {lam})"
    return x, stats


def families(rng, n):
    """(data, penalty): unit noise where most edges are known bends and where pieces are long; a long last piece that runs into the
    free end; integer ties; last runs of one, two and many samples behind a known bend."""
    yield rng.standard_normal(n), 0.1
    yield rng.standard_normal(n), 0.3
    y = rng.standard_normal(n)
    y[-40:] = y[-40]
    yield y, 0.1
    yield rng.integers(-2, 3, n).astype(float), 0.25
    for run in (1, 2, 20):
        y = rng.standard_normal(n)
        y[-run:] = y[-run - 1] + 3.0 + 0.01 * rng.standard_normal(run)     # (a jump of 30 lambda, then `run` samples that stay together)
        yield y, 0.1


def test_the_end_segments_form_gives_the_bits_of_the_general_form(harness, oracle):
    rng = np.random.default_rng(11)
    ends = partial = taken = 0
    for n in LENGTHS:
        for y, lam in families(rng, n):
            for reflect in (False, True):
                x, st = rebuild(harness, y, lam, reflect)
                assert st[0] == 1, (n, st)
                ends, partial, taken = ends + st[0], partial + st[2], taken + st[3]
                if not reflect:
                    truth = oracle.tv1_linearized(y, lam)
                    assert np.max(np.abs(x - truth)) <= 1e-13 * max(1.0, np.max(np.abs(y))), (n, lam, st)
    assert partial >= ends // 2          # (most of the lengths leave a partial last chunk)
    assert taken >= ends // 2            # (... and most end segments are proven: their rows above are the new form's)


def test_every_length_around_a_segment(harness, oracle):
    """Every end-segment length from one sample to two chunks and around a full segment, noise at the headline's penalty."""
    rng = np.random.default_rng(12)
    for n in list(range(1089, 1125)) + list(range(2170, 2180)):
        y = rng.standard_normal(n)
        x, st = rebuild(harness, y, 0.1, True)
        x, st = rebuild(harness, y, 0.1, False)
        truth = oracle.tv1_linearized(y, 0.1)
        assert np.max(np.abs(x - truth)) <= 1e-13 * max(1.0, np.max(np.abs(y))), (n, st)
