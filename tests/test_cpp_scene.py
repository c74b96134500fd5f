"""Scene / updateFromScene of the C++ host facade: tests/cpp/scene_smoke.cpp compiles with plain g++ against the C ABI and
links the product library.  A scene needs the GPU: without one the program must fail loudly, with one it prints the known
counts of a box, a sphere, a cylinder and a cube mesh, rebuilds a field from them and moves the mesh."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpmp2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "scene_smoke.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "scene_smoke")


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
        assert r.returncode == 0 and "\nOK moved" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_facade_rasterizes_known_counts_and_follows_a_moved_mesh_on_gpu():
    r = _run()
    assert r.returncode == 0 and "CELLS box=27 sphere=7 cylinder=25 mesh=27 total=86" in r.stdout, r.stdout + r.stderr
    assert "\nOK moved mesh=27 sphere=0 planar=0,0,0,9" in r.stdout, r.stdout + r.stderr
