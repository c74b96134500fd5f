"""The product's mesh rule (gpmp2_amd/csrc/scene_rule.h) built by the host compiler behind C entry points
(tests/cpp/scene_shim.cpp), so that CPU tests run the kernels' own text."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpmp2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "scene_shim.cpp")
LIB = os.path.join(ROOT, "tests", "cpp", "scene_shim.so")
DEPS = [SRC, os.path.join(CSRC, "scene_rule.h")]

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(LIB) < os.path.getmtime(d) for d in DEPS):
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-shared", "-fPIC",
                                   "-I", CSRC, SRC, "-o", tmp])
            os.replace(tmp, LIB)
        L = C.CDLL(LIB)
        ll, llp, dp = C.c_longlong, C.POINTER(C.c_longlong), C.POINTER(C.c_double)
        L.shim_scene_quantize.argtypes = [C.c_double, llp]
        L.shim_scene_column.argtypes = [llp, ll, ll, dp, llp, llp]
        L.shim_scene_floor_cell.argtypes = [ll]
        L.shim_scene_floor_cell.restype = ll
        L.shim_scene_ceil_cell.argtypes = [ll]
        L.shim_scene_ceil_cell.restype = ll
        _lib = L
    return _lib


def quantize(g):
    """-> q, or None when the guard fires"""
    q = C.c_longlong(0)
    return q.value if lib().shim_scene_quantize(float(g), C.byref(q)) else None


def column(P, Y, Z):
    """P: three fixed-point vertices -> 'skip' (a == 0), None (no crossing) or first = ceil(x); and (e, a) beside it"""
    p = (C.c_longlong * 9)(*[int(x) for v in P for x in v])
    first, e, a = C.c_double(0.0), (C.c_longlong * 3)(), C.c_longlong(0)
    rc = lib().shim_scene_column(p, int(Y), int(Z), C.byref(first), e, C.byref(a))
    if rc < 0:
        return "skip", None
    return (first.value if rc else None), (list(e), a.value)


def floor_cell(v):
    return lib().shim_scene_floor_cell(int(v))


def ceil_cell(v):
    return lib().shim_scene_ceil_cell(int(v))
