"""The 16-byte pieces in which the four wavefronts of k_linearize_arm store the point records of a chunk
(gpmp2_amd/csrc/rec_pieces.h), built by the host compiler behind C entry points (tests/cpp/rec_pieces_shim.cpp), so that
a CPU test runs the text the kernel runs: for the records of D = 1 .. 7 joints (RECL = 3 .. 36 values, odd and even) and
chunks of 1, 2, 25, 63 and 64 live points, every (point, pair) of a live point is produced exactly once by the kernel's
loop over 256 threads, none of a dead point, at the address the point-major layout gives it."""
import ctypes as C
import os
import subprocess
from collections import Counter

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpmp2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "rec_pieces_shim.cpp")
LIB = os.path.join(ROOT, "tests", "cpp", "rec_pieces_shim.so")
DEPS = [SRC, os.path.join(CSRC, "rec_pieces.h")]

RECLS = [D * (D + 1) // 2 + D + 1 for D in range(1, 8)]
POPULATIONS = [1, 2, 25, 63, 64]
THREADS = 256


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(LIB) or any(os.path.getmtime(LIB) < os.path.getmtime(d) for d in DEPS):
        tmp = LIB + f".{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-I", CSRC, SRC, "-o", tmp])
        os.replace(tmp, LIB)
    L = C.CDLL(LIB)
    L.shim_rec_piece.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.shim_rec_piece.restype = C.c_long
    return L


def piece(shim, e, RECL, RECS):
    out = (C.c_int * 4)()
    dst = shim.shim_rec_piece(e, RECL, RECS, out)
    return dict(point=out[0], pair=out[1], padded=bool(out[2]), src=out[3], dst=dst)


def kernel_pieces(shim, P, p_lo, RECL, RECS):
    """the pieces the kernel's store loop produces for the chunk that starts at point p_lo: thread t takes t, t + 256, ..."""
    npc = shim.shim_rec_piece_count(shim.shim_rec_live_points(P, p_lo), RECL)
    nit = (64 * shim.shim_rec_npieces(RECL) + THREADS - 1) // THREADS
    return [piece(shim, t + THREADS * it, RECL, RECS) for it in range(nit) for t in range(THREADS) if t + THREADS * it < npc]


def test_record_lengths_are_those_of_one_to_seven_joints():
    assert RECLS == [3, 6, 10, 15, 21, 28, 36]


def test_live_points_of_a_chunk(shim):
    for p_lo in (0, 64, 128):
        for live in POPULATIONS:
            assert shim.shim_rec_live_points(p_lo + live, p_lo) == live
        assert shim.shim_rec_live_points(p_lo + 65, p_lo) == 64 and shim.shim_rec_live_points(p_lo + 1000, p_lo) == 64
        assert shim.shim_rec_live_points(p_lo, p_lo) == 0 and shim.shim_rec_live_points(p_lo - 3, p_lo) == 0


@pytest.mark.parametrize("RECL", RECLS)
@pytest.mark.parametrize("live", POPULATIONS)
def test_every_pair_of_a_live_point_once_at_its_address(shim, RECL, live):
    npieces = (RECL + 1) // 2
    assert shim.shim_rec_npieces(RECL) == npieces
    for RECS in (2 * npieces, 2 * npieces + 36):      # arm plans; a wider record stride (entries behind G | g | e)
        for p_lo in (0, 64):
            got = kernel_pieces(shim, p_lo + live, p_lo, RECL, RECS)
            seen = Counter((pc["point"], pc["pair"]) for pc in got)
            assert set(seen.values()) == {1}
            assert sorted(seen) == [(pt, pr) for pt in range(live) for pr in range(npieces)]     # no dead point
            for pc in got:
                # present layout: the record of point pt starts pt * RECS doubles behind the chunk's first, value k at + k
                assert pc["dst"] == pc["point"] * RECS + 2 * pc["pair"]
                assert pc["dst"] % 2 == 0 and pc["dst"] + 1 < (pc["point"] + 1) * RECS       # one aligned 16-B piece inside it
                assert pc["padded"] == (2 * pc["pair"] + 1 == RECL)      # the 0.0 pad: last pair of an odd RECL only
    if RECL % 2 == 0:
        assert not any(pc["padded"] for pc in got)


@pytest.mark.parametrize("RECL", RECLS)
def test_consecutive_pieces_are_consecutive_memory(shim, RECL):
    RECS = 2 * shim.shim_rec_npieces(RECL)
    assert [piece(shim, e, RECL, RECS)["dst"] for e in range(64 * RECS // 2)] == [2 * e for e in range(64 * RECS // 2)]


@pytest.mark.parametrize("RECL", RECLS)
def test_partial_records_in_lds(shim, RECL):
    stride, npieces = shim.shim_rec_lds_stride(RECL), shim.shim_rec_npieces(RECL)
    assert stride >= RECL and stride % 2 == 1
    pcs = [piece(shim, e, RECL, 2 * npieces) for e in range(64 * npieces)]
    for pc in pcs:      # the values 2 pair (and 2 pair + 1 unless padded) of the point's own row
        assert pc["src"] == pc["point"] * stride + 2 * pc["pair"]
        assert pc["src"] + (0 if pc["padded"] else 1) < pc["point"] * stride + RECL
    # banks: an 8-byte LDS write goes by its double's index mod 16, an 8-byte read by it mod 32, each over 32 lanes at most.
    # Lanes that write value k of their own point (stride apart) spread over all banks, since the stride is odd.
    assert len({(lane * stride) % 16 for lane in range(16)}) == 16
    # 32 lanes that read 32 consecutive pieces: pieces are two doubles apart, so two lanes per bank is the least any
    # layout of 8-byte reads gives; the value-major layout it replaces put all npieces pieces of a point on one bank
    for base in range(0, 64 * npieces, 32):
        banks = Counter(pc["src"] % 32 for pc in pcs[base:base + 32])
        assert max(banks.values()) <= 2, (RECL, base)
