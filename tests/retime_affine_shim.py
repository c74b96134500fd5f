"""The product's re-timing rule with affine rows (gpmp2_amd/csrc/retime_affine_rule.h) built by the host compiler behind
C entry points (tests/cpp/retime_affine_shim.cpp), so that CPU tests run the kernels' own text."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpmp2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "retime_affine_shim.cpp")
LIB = os.path.join(ROOT, "tests", "cpp", "retime_affine_shim.so")
DEPS = [SRC, os.path.join(CSRC, "retime_rule.h"), os.path.join(CSRC, "retime_affine_rule.h")]

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
        L.shim_retime_affine.argtypes = [i, i, i] + [dp] * 10 + [f, f, f, f] + [dp] * 6
        L.shim_retime_affine.restype = i
        L.shim_row_affine.argtypes = [f, f, f, f, dp]
        L.shim_row_affine.restype = None
        L.shim_row.argtypes = [f, f, f, dp]
        L.shim_row.restype = None
        _lib = L
    return _lib


def _p(x):
    return x.ctypes.data_as(C.POINTER(C.c_double))


def row_affine(cx, cu, off, A):
    """(pl, pu, r, xcap) of retime_row_affine"""
    out = np.zeros(4)
    lib().shim_row_affine(float(cx), float(cu), float(off), float(A), _p(out))
    return out


def row(a, b, A):
    """(pl, pu, r, xcap) of retime_row"""
    out = np.zeros(4)
    lib().shim_row(float(a), float(b), float(A), _p(out))
    return out


def retime_affine(qd, qdd_left, qdd_right, cap, acc, cx_left, cx_right, cu, off, bound, h, max_rate=1.0,
                  rate_start=None, rate_end=None):
    """One row: qd, qdd_left, qdd_right [Md][D], cap [Md], acc [D] or None, cx_left, cx_right, cu, off [Md][R],
    bound [R] -> dict(K, sdot, u, stamps, duration, status, achieved [6]) by retime_affine_row"""
    q, ql, qr = (np.ascontiguousarray(x, dtype=np.float64) for x in (qd, qdd_left, qdd_right))
    Md, D = q.shape
    c = np.ascontiguousarray(cap, dtype=np.float64)
    a = np.full(D, np.inf) if acc is None else np.ascontiguousarray(acc, dtype=np.float64)
    b = np.ascontiguousarray(bound, dtype=np.float64).reshape(-1)
    R = b.shape[0]
    rows = [np.ascontiguousarray(x, dtype=np.float64).reshape(Md, R) for x in (cx_left, cx_right, cu, off)]
    keep = np.zeros(1)      # R = 0: empty arrays have no address worth passing
    ptr = lambda x: _p(x if x.size else keep)   # noqa: E731
    K, sdot, u, stamps = np.zeros((Md, 2)), np.zeros(Md), np.zeros(Md), np.zeros(Md)
    dur, ach = C.c_double(0.0), np.zeros(6)
    st = lib().shim_retime_affine(Md, D, R, _p(q), _p(ql), _p(qr), _p(c), _p(a), *(ptr(x) for x in rows), ptr(b),
                                  float(h), float(max_rate), -1.0 if rate_start is None else float(rate_start),
                                  -1.0 if rate_end is None else float(rate_end), _p(K), _p(sdot), _p(u), _p(stamps),
                                  C.byref(dur), _p(ach))
    return dict(K=K, sdot=sdot, u=u, stamps=stamps, duration=dur.value, status=st, achieved=ach)
