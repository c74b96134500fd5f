"""The random function of the seeded calls on the CPU (no GPU needed): gpmp2_amd/csrc/rng.h through the host compiler
(tests/cpp/rng_shim.cpp) and its numpy restatement (tests/rng_reference.py), held to the Philox4x32-10 known answers, to
each other bit for bit, to the contract that distinct arguments never share a block, and to the moments of a normal."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rng_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpmp2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "rng_shim.cpp")
LIB = os.path.join(ROOT, "tests", "cpp", "rng_shim.so")
DEPS = [SRC, os.path.join(CSRC, "rng.h")]

# counter ; key -> output (Random123 kat_vectors, re-derived from an independent restatement)
KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(LIB) or any(os.path.getmtime(LIB) < os.path.getmtime(d) for d in DEPS):
        tmp = LIB + f".{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-shared", "-fPIC",
                               "-I", os.path.join(ROOT, "include"), "-I", CSRC, SRC, "-o", tmp])
        os.replace(tmp, LIB)
    L = C.CDLL(LIB)
    u32p, vp = C.POINTER(C.c_uint32), C.c_void_p
    L.shim_philox.argtypes = [u32p, u32p, u32p]
    L.shim_philox.restype = None
    L.shim_tuples.argtypes = [C.c_int] + [vp] * 9
    L.shim_tuples.restype = None
    return L


def _tuples(shim, seed, stream, a, b, i, r):
    """-> (counter [n][4], block [n][4], z [n]) of rng.h"""
    n = len(r)
    arrs = [np.ascontiguousarray(seed, dtype=np.uint64)] + \
           [np.ascontiguousarray(x, dtype=np.uint32) for x in (stream, a, b, i)] + [np.ascontiguousarray(r, dtype=np.int32)]
    counter, block, z = np.zeros((n, 4), dtype=np.uint32), np.zeros((n, 4), dtype=np.uint32), np.zeros(n)
    shim.shim_tuples(n, *[x.ctypes.data for x in arrs], counter.ctypes.data, block.ctypes.data, z.ctypes.data)
    return counter, block, z


@pytest.mark.parametrize("ctr,key,want", KNOWN)
def test_known_answers(shim, ctr, key, want):
    c, k, out = (C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), (C.c_uint32 * 4)()
    shim.shim_philox(c, k, out)
    assert tuple(out) == want
    got = ref.philox4x32_10(*ctr, *key)
    assert tuple(int(x) for x in got) == want


def test_shim_and_restatement_agree_bit_for_bit(shim):
    rng = np.random.default_rng(11)
    n = 10_000
    seed = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
    stream = rng.integers(0, 2 ** 24, size=n)
    a, b, i = (rng.integers(0, 2 ** 32, size=n) for _ in range(3))
    r = rng.integers(0, 16, size=n)
    counter, block, z = _tuples(shim, seed, stream, a, b, i, r)
    assert np.array_equal(counter, np.stack(ref.counter(stream, a, b, i, r), axis=1).astype(np.uint32))
    assert np.array_equal(block, np.stack(ref.block(seed, stream, a, b, i, r), axis=1).astype(np.uint32))
    # the normals: the same integers through two libms
    zr = ref.normal(seed, stream, a, b, i, r)
    assert np.all(np.isfinite(z)) and np.abs(z - zr).max() <= 1e-14


def test_distinct_arguments_never_share_a_counter(shim):
    grid = np.array([(s, a, b, i, r) for s in (1, 2) for a in range(3) for b in range(3) for i in range(4)
                     for r in range(15)])
    s, a, b, i, r = grid.T
    counter, _, _ = _tuples(shim, np.zeros(len(r)), s, a, b, i, r)
    seen = {}
    for row, c in zip(grid, map(bytes, counter)):
        seen.setdefault(c, []).append(tuple(int(x) for x in row))
    for members in seen.values():     # a counter is read by one coordinate, or by the two members of one pair
        assert len(members) <= 2
        if len(members) == 2:
            (x, y) = members
            assert x[:4] == y[:4] and abs(x[4] - y[4]) == 4 and (min(x[4], y[4]) & 4) == 0
    assert len(seen) == 2 * 3 * 3 * 4 * 8      # r = 0..14: seven full pairs and the cosine member of {11, 15}


@pytest.mark.parametrize("seed", [2024, 0, 1])
def test_moments_of_the_restatement(seed):
    z = ref.normal_fill(seed, ref.RESTARTS, 0, 1024, 0, 1, 64, 16).ravel()
    n = z.size
    assert n == 2 ** 20
    m, v = abs(z.mean()) * np.sqrt(n), abs(z.var() - 1.0) / np.sqrt(2.0 / n)
    print(f"seed {seed}: |mean| sqrt(n) = {m:.2f}, |var - 1| / sqrt(2 / n) = {v:.2f}, max |z| = {np.abs(z).max():.3f}")
    assert m <= 5 and v <= 5                       # 5-sigma conditions
    assert np.abs(z).max() <= 8.58 and ref.ZMAX < 8.58
