"""The map from a packed record entry G | g | e to the two row positions whose product feeds it
(gpmp2_amd/csrc/record_entries.h), built by the host compiler behind C entry points (tests/cpp/record_entries_shim.cpp),
so that a CPU test runs the text the accumulate kernels run -- for every D up to MAXD, the second and third entry of a
lane included (all of the second from D = 11 on, the third from D = 15 on), which the robots of the GPU tests do not reach."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpmp2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "record_entries_shim.cpp")
LIB = os.path.join(ROOT, "tests", "cpp", "record_entries_shim.so")
DEPS = [SRC, os.path.join(CSRC, "record_entries.h")]


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(LIB) or any(os.path.getmtime(LIB) < os.path.getmtime(d) for d in DEPS):
        tmp = LIB + f".{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-I", CSRC, SRC, "-o", tmp])
        os.replace(tmp, LIB)
    L = C.CDLL(LIB)
    L.shim_record_entry.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.shim_record_entry.restype = None
    return L


def entry(shim, D, NG, e):
    ea, eb = C.c_int(-1), C.c_int(-1)
    shim.shim_record_entry(D, NG, e, C.byref(ea), C.byref(eb))
    return ea.value, eb.value


def test_max_dof_is_the_public_one(shim):
    import re
    hdr = open(os.path.join(ROOT, "include", "gpmp2mi.h")).read()
    assert shim.shim_max_dof() == int(re.search(r"#define GPMP2MI_MAX_DOF (\d+)", hdr).group(1))


def test_entries_are_the_packed_triangle_then_g_then_e(shim):
    MAXD = shim.shim_max_dof()
    lanes = 64 * shim.shim_rec_slots()
    for D in range(1, MAXD + 1):
        NG = D * (D + 1) // 2
        NE = shim.shim_record_entries(D, NG)
        assert NE == NG + D + 1
        assert NE <= lanes == 192          # the launch guard's condition holds up to MAXD
        want = [(k, k2) for k in range(D) for k2 in range(k, D)]    # G: upper triangle, packed by rows
        want += [(k, D) for k in range(D)]                          # g_k = h_k r
        want += [(D, D)]                                            # e = r r
        got = [entry(shim, D, NG, e) for e in range(NE)]
        assert got == want, D
        assert all(0 <= a <= D and 0 <= b <= D for a, b in got), D


def test_past_the_last_entry_reads_position_zero(shim):
    MAXD = shim.shim_max_dof()
    lanes = 64 * shim.shim_rec_slots()
    for D in range(1, MAXD + 1):
        NG = D * (D + 1) // 2
        NE = shim.shim_record_entries(D, NG)
        for e in range(NE, lanes + 1):
            assert entry(shim, D, NG, e) == (0, 0), (D, e)


def test_second_and_third_slot_are_reached(shim):
    # lane + 64 is an entry from D = 10 on (66 entries), lane + 128 from D = 15 on (136 entries)
    MAXD = shim.shim_max_dof()
    ne = {D: shim.shim_record_entries(D, D * (D + 1) // 2) for D in range(1, MAXD + 1)}
    assert min(D for D in ne if ne[D] > 64) == 10
    assert min(D for D in ne if ne[D] > 128) == 15
    assert MAXD >= 15
