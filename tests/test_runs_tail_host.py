"""The known-runs path of the along-fibre kernel on the segment that holds the fibre's last sample, on the host
(tests/runs_tail_harness.cpp mirrors the four phases of sweep_along_kernel RUNS under `endseg` with the lanes of a wave emulated one after
the other; proxtv_amd/csrc/chunkcore.hpp free_end_edges / free_end_settle): the fibre's end is a free end like its start -- the edge
behind sample len - 1 delimits the last run as a known bend would, nothing past it contributes an edge, a run or a piece, the last run
is a piece by itself if it is one sample long and is walked otherwise, and the records go to rebuild_owned FULL = 3.

What is checked: wherever the end segment is solved run by run its rows carry the bits that the speculative walk's records give through
the same rebuild form (and on noise, where no tie can cut a fibre two ways, the records themselves agree: piece ends, types, the codes
before and behind each chunk); where it falls
back nothing was written; every row of the segment is written exactly once and none past the fibre; the rows are the prox.  Twice, like
the chunk tests: IEEE quotients and the device's table reciprocals.

Engagement, measured with this harness on the very columns tests/test_gpu_runs_tail.py sends to the GPU (unit noise, lambda = 0.1, seed
191, M x 64 for M in GPU_ROWS): 7 of 448 end segments fall back (1.6 %), all for want of a known bend within two samples of the
segment's start; the bar is 10 %."""
import ctypes as C
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from test_along_tail_host import LENGTHS

HERE = os.path.dirname(os.path.abspath(__file__))
SEG, CHUNK = 1088, 17
ALL_LENGTHS = tuple(sorted(set(LENGTHS) | set(range(1089, 1125))))
GPU_ROWS, GPU_SEED = (1110, 2177, 3281, 4080, 4081, 4096, 4097), 191     # (tests/test_gpu_runs_tail.py: the same columns)


@pytest.fixture(scope="module", params=["quotients", "table reciprocals"])
def harness(request):
    out = os.path.join(tempfile.mkdtemp(prefix="ptv_runs_tail_"), "libruns_tail.so")
    flags = ["-DPTV_TABLE_RECIP"] if request.param == "table reciprocals" else []
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", *flags, "-o", out,
                    os.path.join(HERE, "runs_tail_harness.cpp")], check=True)
    lib = C.CDLL(out)
    lib.host_runs_tail.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def tail(lib, y, lam, records=False):
    y = np.ascontiguousarray(y, dtype=np.float64)
    x = np.full(y.size, np.nan)
    st = np.zeros(12, dtype=np.int32)
    rc = lib.host_runs_tail(y.ctypes.data, lam, y.size, x.ctypes.data, st.ctypes.data)
    assert rc == 0, f"{-rc} rows differ from the speculative records' / are not written exactly once (len {y.size}, lambda {lam}, {st})"
    # (the records themselves -- piece ends, types, codes -- are compared where no tie can cut a fibre two ways: a knot with a jump of zero
    #  is a piece end to the rule for two-sample runs and none to the walk, or the other way round, and the rows carry the same bits)
    assert not records or st[10] == 0, f"{st[10]} chunk records differ from the speculative walk's (len {y.size}, lambda {lam}, {st})"
    assert st[11] == 0, f"{st[11]} free-end marks disagree with their runs (len {y.size}, lambda {lam}, {st})"
    assert st[0] + st[1] == 1, st          # (one end segment a fibre: solved or fallen back)
    return x, st


def check(lib, oracle, y, lam, what, records=False):
    x, st = tail(lib, y, lam, records)
    truth = oracle.tv1_linearized(y, lam)
    assert np.max(np.abs(x - truth)) <= 1e-13 * max(1.0, np.max(np.abs(y))), (what, y.size, lam, st)
    return st


def last_run(rng, n, run, lam=0.1):
    """Unit noise, then a jump of 30 lambda and `run` samples that stay together: a last run of exactly `run` samples."""
    y = rng.standard_normal(n)
    y[-run:] = y[-run - 1] + 30.0 * lam + 0.01 * rng.standard_normal(run)
    return y


def test_unit_noise_at_every_length(harness, oracle):
    """lambda = 0.1 on N(0, 1): an end segment of one sample, less than a chunk, whole chunks only, a partial last chunk, a full segment."""
    rng = np.random.default_rng(21)
    solved = compared = 0
    for n in ALL_LENGTHS:
        for t in range(3):
            st = check(harness, oracle, rng.standard_normal(n), 0.1, "noise", records=True)
            solved, compared = solved + st[0], compared + st[9]
            assert st[3] <= 64
    assert solved >= 0.9 * 3 * len(ALL_LENGTHS)
    assert compared >= 0.8 * solved       # (most solved segments have every speculative link proven: their bits were compared)


def test_short_last_runs_and_the_cap(harness, oracle):
    """Last runs of 1, 2, 3 and 14 samples behind a planted jump are solved (one sample: a piece by itself; the others walked, however
    short); 15 samples exceed what a lane takes and a constant tail of 40 has no bend in reach: the segment falls back."""
    rng = np.random.default_rng(22)
    inside = solved = 0
    for n in ALL_LENGTHS:
        inseg = n - SEG * ((n - 1) // SEG)          # samples of the end segment
        for run in (1, 2, 3, 14, 15):
            st = check(harness, oracle, last_run(rng, n, run), 0.1, f"last run of {run}")
            if run == 15:
                assert st[1] == 1 and st[4] + st[5] >= 1, (n, run, st)
            elif inseg >= run + 3:                  # (the run and the bend before it lie in the end segment)
                # the last run is never the reason to fall back -- but for the cap that interior segments have as well: a lane's mask holds
                # 13 edges behind its chunk, so a run of 14 samples that starts on a chunk's last row is longer than its lane takes
                if run == 14 and (inseg - run) % CHUNK == CHUNK - 1:
                    assert st[1] == 1 and st[5] >= 1, (n, run, st)
                    continue
                assert st[5] == 0 and st[7] == 0, (n, run, st)
                inside, solved = inside + 1, solved + st[0]
        y = rng.standard_normal(n)
        y[-40:] = y[-40]
        st = check(harness, oracle, y, 0.1, "constant tail")
        assert st[1] == 1 and st[4] + st[5] >= 1, (n, st)
    assert inside > 100 and solved >= 0.9 * inside   # (the rest: no known bend within two samples of the segment's start, 1 % on noise)
    # a last run that starts before the end segment comes in through lane 0's edges before the segment, or sends it back
    for n, run in ((1089, 3), (1090, 3), (1090, 14), (1096, 14), (2177, 2), (2178, 3)):
        check(harness, oracle, last_run(rng, n, run), 0.1, "run from before the segment")


def test_integer_ties(harness, oracle):
    rng = np.random.default_rng(23)
    solved = 0
    for n in ALL_LENGTHS:
        solved += check(harness, oracle, rng.integers(-2, 3, n).astype(float), 0.25, "integers")[0]
    assert solved >= 5


def test_slivers_at_the_free_end(harness, oracle):
    """Jumps of exactly 0, 2 lambda, 4 lambda and 4 lambda (1 +- 6e-9) on the last two edges of the fibre, either sign, behind a known
    bend of either type: the rule for two-sample runs must not reach across the free end, and an edge within rounding of 4 lambda is a
    bend to the masks exactly when it is one to the walk (profiles/NOTES_r06.md, the sliver case, set at the free end).
    "Exactly" needs numbers in which it can be said: penalties of 1/4 and 1/8 on samples that are multiples of 2^-12, so that 2 lambda
    and 4 lambda are jumps of the data to the last bit.  (At lambda = 0.1 a jump meant to be 2 lambda comes out as 0.20000000000000018:
    a tie decided by rounding, which the rule for two-sample runs and the walk may cut differently -- a knot with a jump of zero, one
    ulp between the two cuts, 1 case in 1200 -- as they may on interior segments: tests/test_runs_host.py, late iterates.)"""
    rng = np.random.default_rng(24)
    jumps = [0.0, 2.0, 4.0, 4.0 * (1 + 6e-9), 4.0 * (1 - 6e-9)]
    solved = 0
    for n in (1110, 2177, 4096, 1091, 1105, 1106):
        for lam in (0.125, 0.25):
            for (j1, j2), (s0, s1, s2) in itertools.product(itertools.product(jumps, jumps), itertools.product((-1.0, 1.0), repeat=3)):
                y = np.round(rng.standard_normal(n) * 2.0 * 4096.0) / 4096.0
                y[-3] = y[-4] + s0 * np.round((5.0 + rng.random()) * lam * 4096.0) / 4096.0     # the preceding bend, known a priori: CEIL or FLOOR
                y[-2] = y[-3] + s1 * j1 * lam
                y[-1] = y[-2] + s2 * j2 * lam
                solved += check(harness, oracle, y, lam, f"sliver {j1} {j2} {s0} {s1} {s2}")[0]
    assert solved > 1000


def test_a_last_run_whose_first_bend_lies_in_the_chunk_before(harness, oracle):
    """The fibre's last chunk holds one to three samples and the last run six to fourteen: the run is listed by the lane before, walked by
    whichever lane its number says, and its piece ends land in two chunks' records."""
    rng = np.random.default_rng(25)
    solved = 0
    for chunks in (1, 3, 20, 63):
        for rows in (1, 2, 3):
            n = SEG + CHUNK * chunks + rows
            for run in (6, 10, 14):
                st = check(harness, oracle, last_run(rng, n, run), 0.1, f"run of {run} over the last chunk boundary")
                solved += st[0]
    assert solved >= 30


def test_engagement_on_the_gpu_tests_columns(harness):
    """The share of end segments that fall back on the columns of tests/test_gpu_runs_tail.py stays under 10 % (the margin
    test_gpu_runs.py uses for interior segments).  Measured: see the module's docstring."""
    rng = np.random.default_rng(GPU_SEED)
    solved = fell = 0
    reasons = np.zeros(5, dtype=np.int64)
    for M in GPU_ROWS:
        X = rng.standard_normal((M, 64))
        for c in range(64):
            _, st = tail(harness, X[:, c], 0.1, records=True)
            solved, fell = solved + st[0], fell + st[1]
            reasons += st[4:9]
    print(f"end segments: {solved} solved run by run, {fell} fallen back ({100.0 * fell / (solved + fell):.1f} %), reasons {reasons.tolist()}")
    assert solved + fell == 64 * len(GPU_ROWS)
    assert fell < 0.1 * (solved + fell)
