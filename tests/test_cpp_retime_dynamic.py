"""The RetimeTrajectory overload that takes an ArmDynamics / the SelectBestTrajectory overload of its results in the C++
host facade: tests/cpp/retime_dynamic_smoke.cpp compiles with plain g++ against the C ABI and links the product library.
The selection rule runs without a GPU; the profile must fail loudly without one, and with one give the closed form of the
planar two-link arm at rest, torques within their limits on a line, and the bits of the plain RetimeTrajectory without
limits."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpmp2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "retime_dynamic_smoke.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "retime_dynamic_smoke")


def _build():
    newest = max(os.path.getmtime(p) for p in (SRC, os.path.join(ROOT, "include", "gpmp2mi_planner.hpp"),
                                               os.path.join(ROOT, "include", "gpmp2mi.h")))
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < newest:
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE,
                               "-L", CSRC, "-lgpmp2mi", f"-Wl,-rpath,{CSRC}"])
    return EXE


def _run():
    return subprocess.run([_build()], capture_output=True, text=True, timeout=300)


def test_selection_runs_everywhere_and_the_profile_fails_loudly_without_gpu():
    from gpmp2_amd import engine
    r = _run()
    assert r.stdout.startswith("SELECT OK"), r.stdout + r.stderr
    if engine.Engine().device_count() == 0:
        assert r.returncode == 3 and "EXCEPTION" in r.stdout and "no usable HIP device" in r.stdout, r.stdout + r.stderr
    else:
        assert r.returncode == 0 and "\nOK best=" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_facade_retimes_under_torque_limits_and_selects_on_gpu():
    r = _run()
    assert r.returncode == 0 and "LINE" in r.stdout and "\nOK best=" in r.stdout, r.stdout + r.stderr
