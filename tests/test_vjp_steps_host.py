"""The step codes of the prox derivative without a GPU: chunk_codes / chunk_load_steps of proxtv_amd/csrc/vjpcore.hpp, compiled for
the host by tests/vjp_steps_host.cpp.  A chunk filled from its code word is the chunk filled from y, so phases A, B and C from the
words give the bits they give from y -- there is no tolerance anywhere in this file."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import vjp_model as vm

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "vjp_steps_host.cpp")
CHUNKS = (1, 2, 7, 16)
LENGTHS = (1, 2, 3, 7, 15, 16, 17, 33, 112, 113, 300)     # 112 = lcm(1, 2, 7, 16): every chunking ends on a full chunk, 113 one past it
GXX = ["g++", "-O2", "-std=c++17", "-ffp-contract=off"]


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(tempfile.mkdtemp(prefix="ptv_vjp_steps_"), "libvjp_steps_host.so")
    subprocess.run(GXX + ["-fPIC", "-shared", "-o", out, SRC], check=True)
    lib = C.CDLL(out)
    lib.vjp_steps_host_compare.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.vjp_steps_host_words.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.vjp_steps_host_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def fibres():
    """(name, y, g): random fibres, random piecewise-constant ones, all-equal and strictly monotone ones (both ways), every length."""
    rng = np.random.default_rng(2027)
    for n in LENGTHS:
        g = rng.standard_normal(n)
        yield f"random n{n}", rng.standard_normal(n), g
        yield f"piecewise constant n{n}", np.repeat(rng.standard_normal(n), rng.integers(1, 9, n))[:n], g
        yield f"all equal n{n}", np.full(n, 0.75), g
        yield f"monotone up n{n}", np.cumsum(rng.uniform(0.1, 1.0, n)), g
        yield f"monotone down n{n}", -np.cumsum(rng.uniform(0.1, 1.0, n)), g
    # jumps the rule calls no step, between jumps it calls steps: the words must say what is_step says, not what != says
    y = np.repeat(rng.standard_normal(40), 5) + np.tile([0.0, 1e-11, -1e-11, 2e-11, 0.0], 40)
    yield "sub-threshold ripple", y, rng.standard_normal(y.size)


def words_of(lib, y, chunk):
    words = np.zeros((y.size + chunk - 1) // chunk, dtype=np.uint32)
    assert lib.vjp_steps_host_words(y.ctypes.data, y.size, chunk, words.ctypes.data) == words.size
    return words


def run(lib, y, words, g, chunk):
    gx, gw = np.full(g.size, np.nan), np.full(max(g.size - 1, 0), np.nan)
    nseg = lib.vjp_steps_host_run(None if y is None else y.ctypes.data, None if words is None else words.ctypes.data, g.ctypes.data, g.size,
                                  chunk, gx.ctypes.data, gw.ctypes.data)
    assert nseg >= 1, chunk
    return gx, gw, nseg


def test_a_chunk_from_its_word_is_the_chunk_from_y(harness):
    """step, up, len, has_next and the cotangents of chunk_load_steps(chunk_codes(y)) against chunk_load(y), chunk by chunk; in the same
    pass the harness checks that the bits beyond the owned edges are 0 and that up lies inside step."""
    for name, y, g in fibres():
        for chunk in CHUNKS:
            assert harness.vjp_steps_host_compare(y.ctypes.data, g.ctypes.data, y.size, chunk) == 0, (name, chunk)
    assert harness.vjp_steps_host_compare(y.ctypes.data, g.ctypes.data, y.size, 64) == -1      # (a word holds 16 edges)


def test_the_words_are_the_documented_format(harness):
    """Bit k of a word: the edge behind sample k of the chunk is a step by the numpy model's rule; bit 16 + k: it goes up.  Everything
    else is 0: beyond a short last chunk, behind the fibre's last sample, and the up bit of an edge that is no step."""
    for name, y, _ in fibres():
        n = y.size
        step = np.zeros(n, dtype=bool)
        step[:n - 1] = vm.steps(y)
        up = np.zeros(n, dtype=bool)
        up[:n - 1] = step[:n - 1] & (np.diff(y) > 0)
        for chunk in CHUNKS:
            words = words_of(harness, y, chunk)
            want = np.zeros_like(words)
            for k in range(n):
                want[k // chunk] |= np.uint32((int(step[k]) | (int(up[k]) << 16)) << (k % chunk))
            assert np.array_equal(words, want), (name, chunk)
            assert not np.any((words >> 16) & ~words & 0xffff), (name, chunk)
            assert sum(bin(int(w) & 0xffff).count("1") for w in words) == int(step.sum()), (name, chunk)
            assert not np.any(words >> (16 + chunk)) and not np.any((words & 0xffff) >> chunk), (name, chunk)


def test_the_pipeline_from_words_gives_the_bits_of_the_pipeline_from_y(harness):
    for name, y, g in fibres():
        for chunk in CHUNKS:
            gx, gw, nseg = run(harness, y, None, g, chunk)
            gx2, gw2, nseg2 = run(harness, None, words_of(harness, y, chunk), g, chunk)
            assert nseg2 == nseg == 1 + int(vm.steps(y).sum()), (name, chunk)
            assert np.array_equal(gx2, gx) and np.array_equal(gw2, gw), (name, chunk)
            assert not np.any(np.isnan(gx)) and not np.any(np.isnan(gw)), (name, chunk)


def test_the_harness_as_a_program_under_the_sanitizers():
    """The same checks on fibres the program draws itself, built once with -fsanitize=address,undefined and run as its own process."""
    exe = os.path.join(tempfile.mkdtemp(prefix="ptv_vjp_steps_san_"), "vjp_steps_host")
    subprocess.run(GXX + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DVJP_STEPS_MAIN", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "VJP_STEPS_HOST_OK" in r.stdout
