"""integratePoints / integrateDepth / refreshFromEvidence / evidence of the field classes of the C++ host facade:
tests/cpp/sensor_smoke.cpp compiles with plain g++ against the C ABI and links the product library.  A field needs the
GPU: without one the program must fail loudly, with one it marks a plate from a frame of rays, carves it away again with
two frames that pass through it, and takes a depth image."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpmp2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "sensor_smoke.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "sensor_smoke")


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
        assert r.returncode == 0 and "\nOK depth" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_facade_marks_and_carves_a_plate_on_gpu():
    r = _run()
    assert r.returncode == 0 and "CARVED before=0.500 hit=-0.100 after=0.200 occupied=9" in r.stdout, r.stdout + r.stderr
    assert "\nOK depth hit=8 max_range=1 occupied=8" in r.stdout, r.stdout + r.stderr
