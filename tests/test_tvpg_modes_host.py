"""The load / store functors of tvpvjp::solve (proxtv_amd/csrc/tvpvjpcore.hpp) without a GPU: tests/tvpg_modes_host.cpp, a
stand-alone program, runs every write-out MODE of the reverse recurrences through the functors -- on the arrays as the solvers alias
them -- against the plain call followed by the write-out in plain C++, and requires equal bits: lengths 1, 2, 7, 8, 9, 17, 129, both
arms, the mean branch, strides 1 and 3."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def test_every_mode_through_the_functors_gives_the_bits_of_plain_then_write_out():
    exe = os.path.join(tempfile.mkdtemp(prefix="ptv_tvpg_modes_"), "tvpg_modes_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "tvpg_modes_host.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "MODES_HOST_OK" in r.stdout
