"""The host driver's workspace carver, staging rule and stage layouts (gpmp2_amd/csrc/host/staging.h), built by the host
compiler behind C entry points (tests/cpp/staging_shim.cpp), so that CPU tests run the driver's own text."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpmp2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "staging_shim.cpp")
LIB = os.path.join(ROOT, "tests", "cpp", "staging_shim.so")
DEPS = [SRC, os.path.join(CSRC, "host", "staging.h")]


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(LIB) or any(os.path.getmtime(LIB) < os.path.getmtime(d) for d in DEPS):
        tmp = LIB + f".{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-I", CSRC, SRC, "-o", tmp])
        os.replace(tmp, LIB)
    L = C.CDLL(LIB)
    z, zp = C.c_size_t, C.POINTER(C.c_size_t)
    L.shim_carve_rows.argtypes = [C.c_int, zp, C.c_void_p, zp, zp]
    L.shim_carve_rows.restype = None
    L.shim_staging_rule.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.shim_staging_rule.restype = C.c_void_p
    L.shim_stage_bytes.argtypes = [C.c_int] + [z] * 7
    L.shim_stage_bytes.restype = z
    return L


def carve(shim, sizes, base):
    n = len(sizes)
    off, total = (C.c_size_t * n)(), C.c_size_t(0)
    shim.shim_carve_rows(n, (C.c_size_t * n)(*sizes), base, off, C.byref(total))
    return list(off), total.value


def test_carving_goes_by_offsets_whatever_the_base(shim):
    sizes = [0, 1, 255, 256, 257, 0, 1]
    rounded = [(s + 255) // 256 * 256 for s in sizes]
    assert rounded == [0, 256, 256, 256, 512, 0, 256]
    block = C.create_string_buffer(sum(rounded) + 1)
    off_null, total_null = carve(shim, sizes, None)
    off_real, total_real = carve(shim, sizes, C.addressof(block))
    assert off_null == off_real == [sum(rounded[:i]) for i in range(len(sizes))]
    assert all(o % 256 == 0 for o in off_null)
    assert total_null == total_real == sum(rounded)


def test_staging_rule(shim):
    caller, staged = 0x1000, 0x2000
    assert shim.shim_staging_rule(0, caller, staged) == caller    # a device form writes the caller's array
    assert shim.shim_staging_rule(0, None, staged) is None        # ... and nothing where there is none
    assert shim.shim_staging_rule(1, caller, staged) == staged    # a host form writes the staged one
    assert shim.shim_staging_rule(1, None, staged) is None        # ... and computes only what the caller asked for


# What plan_ws_layout(nullptr, ...).bytes of each stage's unit gave at B = 3, N = 2, D = 2, inter_step = 1 (S = 2 spheres,
# max_alt = 2) in the commit before the units' layouts moved into staging.h, printed by a scratch program built from
# that commit; next to them the bytes of the stage's records at that shape (3 rows of one block: ScoreRec 40 bytes,
# MotionRec 72, PathRec 48), the words of a bit-matrix row and GPMP2MI_MAX_ALTERNATIVES, from the same program.
PARENT_BYTES = [
    ("score", 0, 120, 0, 2304),
    ("self", 1, 120, 120, 2560),
    ("motion", 2, 216, 0, 3840),
    ("moving", 3, 120, 0, 3328),
    ("path", 4, 144, 0, 3072),
    ("retime", 5, 0, 0, 5376),
    ("group", 6, 1, 64, 4096),
]


@pytest.mark.parametrize("name,stage,rec,rec2,expected", PARENT_BYTES, ids=[c[0] for c in PARENT_BYTES])
def test_stage_layouts_did_not_drift(shim, name, stage, rec, rec2, expected):
    assert shim.shim_stage_bytes(stage, 3, 2, 2, 1, rec, rec2, 2) == expected
