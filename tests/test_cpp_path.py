"""The workspace path through the plain C header: tests/cpp/path_smoke.cpp compiles with plain g++ against
include/gpmp2mi.h and links the product library.  A field needs the GPU: without one the program must fail loudly, with
one it plans a planar arm along a straight tool line, checks and selects, and plans again with the path cleared."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpmp2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "path_smoke.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "path_smoke")


def _build():
    newest = max(os.path.getmtime(p) for p in (SRC, os.path.join(ROOT, "include", "gpmp2mi.h")))
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < newest:
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE,
                               "-L", CSRC, "-lgpmp2mi", f"-Wl,-rpath,{CSRC}"])
    return EXE


def _run():
    return subprocess.run([_build()], capture_output=True, text=True, timeout=300)


def test_smoke_builds_and_fails_loudly_without_gpu():
    from gpmp2_amd import engine
    r = _run()
    if engine.Engine().device_count() == 0:
        assert r.returncode == 3 and "EXCEPTION" in r.stdout and "no usable HIP device" in r.stdout, r.stdout + r.stderr
    else:
        assert r.returncode == 0 and "\nOK path" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_smoke_follows_the_line_on_gpu():
    r = _run()
    assert r.returncode == 0 and "\nOK path" in r.stdout, r.stdout + r.stderr
    assert "WITH max_pos_dev" in r.stdout and " of 2\nWITHOUT" in r.stdout, r.stdout + r.stderr
