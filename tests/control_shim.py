"""The product's step-control rules and cyclic-reduction schedule (gpmp2_amd/csrc/step_control.h, cr_schedule.h) built
by the host compiler behind C entry points (tests/cpp/control_shim.cpp), so that CPU tests run the kernels' own text."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpmp2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "control_shim.cpp")
LIB = os.path.join(ROOT, "tests", "cpp", "control_shim.so")
DEPS = [SRC, os.path.join(CSRC, "step_control.h"), os.path.join(CSRC, "cr_schedule.h")]

OPT_GN, OPT_LM, OPT_DOGLEG = 0, 1, 2
RETURNED, MOVED, RETRY, NOT_SPD = 1, 2, 4, 8     # flags of a trial step's outcome


class StepRules(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("opt_type", "max_iter", "no_increase", "fixed_iters")] + \
               [(k, C.c_double) for k in ("rel_thresh", "abs_tol", "err_tol", "lm_lambda0", "lm_factor", "lm_upper", "lm_lower",
                                          "lm_min_fidelity", "dl_delta0")]


def rules_of(setting, fixed_iters=0):
    """the StepRules a plan makes of a TrajOptimizerSetting (host/plan_create.hip)"""
    from gpmp2_amd import _capi
    s, o, keep = _capi.make_settings(setting)
    return StepRules(s.opt_type, s.max_iter, s.final_iter_no_increase, fixed_iters, s.rel_thresh, o.abs_error_tol, o.error_tol,
                     o.lm_lambda_initial, o.lm_lambda_factor, o.lm_lambda_upper, o.lm_lambda_lower, o.lm_min_model_fidelity,
                     o.dogleg_delta_initial)


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(LIB) < os.path.getmtime(d) for d in DEPS):
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-shared", "-fPIC",
                                   "-I", os.path.join(ROOT, "include"), "-I", CSRC, SRC, "-o", tmp])
            os.replace(tmp, LIB)
        L = C.CDLL(LIB)
        d, i, ip, dp, rp = C.c_double, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(StepRules)
        L.shim_check_convergence.argtypes = [d, d, d, d, d]
        L.shim_first_decide.argtypes = [rp, d, ip]
        L.shim_loop_decide.argtypes = [rp, i, i, d, d, ip]
        L.shim_gn_decide.argtypes = [rp, i, d, d, ip]
        L.shim_gn_iterate.argtypes = [i]
        L.shim_lm_try_lambda.argtypes = [rp, d, d, d, d, d, i, dp]
        L.shim_dogleg_iterate.argtypes = [d, d, d, d, d, i, dp]
        L.shim_dogleg_blend.argtypes = [d, d, d, d, d, dp]
        L.shim_dogleg_blend.restype = None
        L.shim_cr_hfinal.argtypes = [i]
        L.shim_cr_level.argtypes = [i, i, i, ip, ip, ip]
        L.shim_cr_back_count.argtypes = [i, i]
        L.shim_cr_back_block.argtypes = [i, i, i]
        _lib = L
    return _lib


# ------------------------------------------------------------------------------- step control
def first_decide(rules, err):
    st = C.c_int(-1)
    return lib().shim_first_decide(C.byref(rules), err, C.byref(st)), st.value


def loop_decide(rules, it, counted, prev, err_after):
    st = C.c_int(-1)
    return lib().shim_loop_decide(C.byref(rules), it, int(counted), prev, err_after, C.byref(st)), st.value


def gn_decide(rules, it, prev, new_err):
    st = C.c_int(-1)
    return lib().shim_gn_decide(C.byref(rules), it, prev, new_err, C.byref(st)), st.value


def gn_iterate(failed):
    return lib().shim_gn_iterate(int(failed))


def lm_try_lambda(rules, lam, cur_err, new_err, gd, dd, failed=False):
    """-> (flags, lambda afterwards)"""
    out = C.c_double()
    return lib().shim_lm_try_lambda(C.byref(rules), lam, cur_err, new_err, gd, dd, int(failed), C.byref(out)), out.value


def dogleg_iterate(Delta, cur_err, new_err, q, xnorm, failed=False):
    """-> (flags, trust radius afterwards)"""
    out = C.c_double()
    return lib().shim_dogleg_iterate(Delta, cur_err, new_err, q, xnorm, int(failed), C.byref(out)), out.value


def dogleg_blend(gg, gHg, gn, nn, Delta):
    """-> cu, cn, q"""
    out = (C.c_double * 3)()
    lib().shim_dogleg_blend(gg, gHg, gn, nn, Delta, out)
    return out[0], out[1], out[2]


# ------------------------------------------------------------------------------- cyclic-reduction schedule
def cr_hfinal(N):
    return lib().shim_cr_hfinal(N)


def cr_level(N, h, updates=True):
    """-> [(kind, block)] of the level's tasks in task order, (countE, countU, final)"""
    elim, block, counts = (C.c_int * (N + 2))(), (C.c_int * (N + 2))(), (C.c_int * 3)()
    k = lib().shim_cr_level(N, h, int(updates), elim, block, counts)
    assert k == counts[0] + counts[1] <= N + 2
    return [("E" if elim[t] else "U", block[t]) for t in range(k)], (counts[0], counts[1], bool(counts[2]))


def cr_back_count(N, h):
    return lib().shim_cr_back_count(N, h)


def cr_back_block(N, h, idx):
    return lib().shim_cr_back_block(N, h, idx)
