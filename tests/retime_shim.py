"""The product's re-timing rule (gpmp2_amd/csrc/retime_rule.h) built by the host compiler behind a C entry point
(tests/cpp/retime_shim.cpp), so that CPU tests run the kernels' own text."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpmp2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "retime_shim.cpp")
LIB = os.path.join(ROOT, "tests", "cpp", "retime_shim.so")
DEPS = [SRC, os.path.join(CSRC, "retime_rule.h")]

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
        i, f, dp = C.c_int, C.c_double, C.POINTER(C.c_double)
        L.shim_retime_path.argtypes = [i, i, dp, dp, dp, dp, dp, f, f, f, f, dp, dp, dp, dp, dp, dp]
        L.shim_retime_path.restype = i
        _lib = L
    return _lib


def retime_path(qd, qdd_left, qdd_right, cap, acc, h, max_rate=1.0, rate_start=None, rate_end=None):
    """One row [Md][D] -> dict(K, sdot, u, stamps, duration, status, achieved) by retime_path_row; acc None: no limit"""
    q, ql, qr = (np.ascontiguousarray(x, dtype=np.float64) for x in (qd, qdd_left, qdd_right))
    Md, D = q.shape
    c = np.ascontiguousarray(cap, dtype=np.float64)
    a = np.full(D, np.inf) if acc is None else np.ascontiguousarray(acc, dtype=np.float64)
    K, sdot, u, stamps = np.zeros((Md, 2)), np.zeros(Md), np.zeros(Md), np.zeros(Md)
    dur, ach = C.c_double(0.0), np.zeros(4)
    p = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    st = lib().shim_retime_path(Md, D, p(q), p(ql), p(qr), p(c), p(a), float(h), float(max_rate),
                                -1.0 if rate_start is None else float(rate_start),
                                -1.0 if rate_end is None else float(rate_end), p(K), p(sdot), p(u), p(stamps),
                                C.byref(dur), p(ach))
    return dict(K=K, sdot=sdot, u=u, stamps=stamps, duration=dur.value, status=st, achieved=ach)
