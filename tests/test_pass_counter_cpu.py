"""The word through which the workgroups of a pass-closing kernel count themselves in (gpmp2_amd/csrc/pass_counter.h):
arrivals in the high half, continuing trajectories in the low half, one atomic add per workgroup.  The header's pure
functions are built by the host compiler (tests/cpp/pass_counter_shim.cpp) and driven through every arrival order that
matters: exactly one arrival must report "last", it must be the final one, and it must decode the true count."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpmp2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "pass_counter_shim.cpp")
LIB = os.path.join(ROOT, "tests", "cpp", "pass_counter_shim.so")
DEPS = [SRC, os.path.join(CSRC, "pass_counter.h")]

GRIDS = [1, 2, 64, 1025]
SHUFFLES = 100


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(LIB) or any(os.path.getmtime(LIB) < os.path.getmtime(d) for d in DEPS):
        tmp = LIB + f".{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-I", CSRC, SRC, "-o", tmp])
        os.replace(tmp, LIB)
    L = C.CDLL(LIB)
    ip = C.POINTER(C.c_int)
    L.shim_pass_arrival.argtypes = [C.c_int]
    L.shim_pass_arrival.restype = C.c_uint64
    L.shim_pass_arrivals_before.argtypes = [C.c_uint64]
    L.shim_pass_arrived_last.argtypes = [C.c_uint64, C.c_int]
    L.shim_pass_count.argtypes = [C.c_uint64, C.c_int]
    L.shim_pass_run.argtypes = [C.c_int, ip, ip, ip, ip, C.POINTER(C.c_uint64)]
    return L


def run(L, order, continues):
    grid = len(order)
    o = np.ascontiguousarray(order, dtype=np.int32)
    c = np.ascontiguousarray(continues, dtype=np.int32)
    ip = C.POINTER(C.c_int)
    who, count, word = C.c_int(), C.c_int(), C.c_uint64()
    lasts = L.shim_pass_run(grid, o.ctypes.data_as(ip), c.ctypes.data_as(ip), C.byref(who), C.byref(count), C.byref(word))
    return lasts, who.value, count.value, word.value


def contributions(grid, rng):
    """the 0 / 1 patterns of a grid: nobody continues, everybody does, and seeded mixtures"""
    yield np.zeros(grid, dtype=np.int32)
    yield np.ones(grid, dtype=np.int32)
    for _ in range(3):
        yield rng.integers(0, 2, size=grid).astype(np.int32)


def orders(grid, rng):
    yield np.arange(grid)
    yield np.arange(grid)[::-1]
    for _ in range(SHUFFLES):
        yield rng.permutation(grid)


def test_encoding(shim):
    assert shim.shim_pass_arrival(0) == 1 << 32
    assert shim.shim_pass_arrival(1) == (1 << 32) + 1
    w = (7 << 32) + 5
    assert shim.shim_pass_arrivals_before(w) == 7
    assert shim.shim_pass_count(w, 1) == 6 and shim.shim_pass_count(w, 0) == 5
    assert shim.shim_pass_arrived_last(w, 8) == 1
    assert shim.shim_pass_arrived_last(w, 7) == 0 and shim.shim_pass_arrived_last(w, 9) == 0
    assert shim.shim_pass_arrived_last(0, 1) == 1   # a grid of one: the first arrival is the last


@pytest.mark.parametrize("grid", GRIDS)
def test_one_last_arrival_with_the_true_count(shim, grid):
    rng = np.random.default_rng(20260 + grid)
    for cont in contributions(grid, rng):
        true = int(cont.sum())
        for order in orders(grid, rng):
            lasts, who, count, word = run(shim, order, cont)
            assert lasts == 1
            assert who == grid - 1          # the arrival that completes the grid, whoever it is
            assert count == true
            assert word == (grid << 32) + true   # nothing carried between the halves


@pytest.mark.parametrize("grid", GRIDS)
def test_extreme_counts(shim, grid):
    """count 0 and count == grid, whichever workgroup arrives last"""
    for value in (0, 1):
        cont = np.full(grid, value, dtype=np.int32)
        for last in {0, grid // 2, grid - 1}:
            order = np.array([w for w in range(grid) if w != last] + [last])
            lasts, who, count, _ = run(shim, order, cont)
            assert (lasts, who, count) == (1, grid - 1, value * grid)
