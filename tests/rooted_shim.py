"""The rooted cyclic-reduction schedule (gpmp2_amd/csrc/cr_schedule.h, crr_*) built by the host compiler behind C entry
points (tests/cpp/rooted_shim.cpp), the way control_shim builds its shim: CPU tests run the kernels' own text."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpmp2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "rooted_shim.cpp")
LIB = os.path.join(ROOT, "tests", "cpp", "rooted_shim.so")
DEPS = [SRC, os.path.join(CSRC, "cr_schedule.h")]

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(LIB) < os.path.getmtime(d) for d in DEPS):
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-I", CSRC, SRC, "-o", tmp])
            os.replace(tmp, LIB)
        L = C.CDLL(LIB)
        i, ip = C.c_int, C.POINTER(C.c_int)
        L.shim_crr_top.argtypes = [i]
        L.shim_crr_levels.argtypes = [i]
        L.shim_cr_hfinal.argtypes = [i]
        L.shim_crr_level.argtypes = [i, i, i, ip, ip, ip]
        L.shim_crr_back_count.argtypes = [i, i]
        L.shim_crr_back_block.argtypes = [i, i, i]
        L.shim_crr_groups.argtypes = [i, i]
        L.shim_chunk_states.argtypes = [i]
        L.shim_crr_window.argtypes = [i, i, i, i, C.POINTER(C.c_ulonglong)]
        _lib = L
    return _lib


def top(N):
    return lib().shim_crr_top(N)


def levels(N):
    return lib().shim_crr_levels(N)


def hfinal(N):
    """the final level of the schedule the wide and dense paths keep"""
    return lib().shim_cr_hfinal(N)


def level(N, h, updates=True):
    """-> [(kind, v)] of the level's tasks in task order, (countE, countU)"""
    elim, block, counts = (C.c_int * (N + 2))(), (C.c_int * (N + 2))(), (C.c_int * 2)()
    k = lib().shim_crr_level(N, h, int(updates), elim, block, counts)
    assert k == counts[0] + counts[1] <= N + 2
    return [("E" if elim[t] else "U", block[t]) for t in range(k)], (counts[0], counts[1])


def back_count(N, h):
    return lib().shim_crr_back_count(N, h)


def back_block(N, h, idx):
    return lib().shim_crr_back_block(N, h, idx)


def groups(N, g):
    return lib().shim_crr_groups(N, g)


def zns():
    """states a chunk of 64 evaluation points may read (k_linearize_arm keeps them in LDS)"""
    return lib().shim_zns()


def fxs():
    """slots of the step window of the fused finish"""
    return lib().shim_fxs()


def chunk_states(I):
    return lib().shim_chunk_states(I)


def window(N, s0, s1, span=None):
    """-> w0, {h: set of tree indices v} for h = 1, 2, 4 (to solve) and 8 (to fetch); span: the kernel's window, FXS"""
    span = fxs() if span is None else span
    out = (C.c_ulonglong * 4)()
    w0 = lib().shim_crr_window(N, s0, s1, span, out)
    return w0, {h: {w0 + k for k in range(64) if (out[t] >> k) & 1} for t, h in enumerate((1, 2, 4, 8))}
