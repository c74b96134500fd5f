"""updateFromOccupancy / updateFromPoints of the two field classes of the C++ host facade: tests/cpp/map_smoke.cpp compiles
with plain g++ against the C ABI and links the product library.  A field needs the GPU: without one the program must fail
loudly, with one it updates a field from points in place and prints a queried distance that changed sign."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpmp2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "map_smoke.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "map_smoke")


def _build():
    newest = max(os.path.getmtime(p) for p in (SRC, os.path.join(ROOT, "include", "gpmp2mi_planner.hpp"),
                                               os.path.join(ROOT, "include", "gpmp2mi.h")))
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < newest:
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE,
                               "-L", CSRC, "-lgpmp2mi", f"-Wl,-rpath,{CSRC}"])
    return EXE


def _run():
    return subprocess.run([_build()], capture_output=True, text=True, timeout=300)


def test_facade_builds_and_fails_loudly_without_gpu():
    from gpmp2_amd import engine
    r = _run()
    if engine.Engine().device_count() == 0:
        assert r.returncode == 3 and "EXCEPTION" in r.stdout and "no usable HIP device" in r.stdout, r.stdout + r.stderr
    else:
        assert r.returncode == 0 and "\nOK after=" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_facade_updates_a_field_from_points_on_gpu():
    r = _run()
    assert r.returncode == 0 and "CHANGED before=0.500 after=-0.200 kept=27 outside=1" in r.stdout, r.stdout + r.stderr
    assert "\nOK after=-0.200" in r.stdout, r.stdout + r.stderr
