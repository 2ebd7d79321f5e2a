"""No-GPU checks of the TV-L2 derivative's boundary, done the way tests/test_cabi_cpu.py does them: the header declares the two entry
points, the built library exports them unmangled, the ctypes table binds them, and the build lists the new unit."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["proxtv_tv2_fibres_dev", "proxtv_tv2_fibres_vjp_dev"]


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "proxtv_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?(?:int|void|double|long|char|Workspace)\s*\**\s*(\w+)\s*\(", text, flags=re.M))


def test_tv2_entry_points_resolve_in_the_built_library():
    from proxtv_amd import _lib
    lib = _lib.load()
    names = declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.split()[1:2] == ["T"]}
    for n in NEW:
        assert n in names, f"include/proxtv_amd.h does not declare {n}"
        assert hasattr(lib, n), f"libproxtv_amd.so does not export {n}"
        assert n in defined, n
        assert n in _lib.SIGNATURES, n
    # mu sits between out and ns; lambda is the last argument before the stream
    assert len(_lib.SIGNATURES["proxtv_tv2_fibres_dev"][1]) == 8 and len(_lib.SIGNATURES["proxtv_tv2_fibres_vjp_dev"][1]) == 10


def test_the_build_lists_the_new_unit():
    from proxtv_amd import build
    assert "tv2_vjp" in build.PLAIN_UNITS
    assert os.path.exists(os.path.join(os.path.dirname(build.__file__), "csrc", "tv2_vjp.hip"))
    assert os.path.exists(os.path.join(os.path.dirname(build.__file__), "csrc", "tv2vjpcore.hpp"))

