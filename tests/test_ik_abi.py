"""The "goal configurations" section of include/gpmp2mi.h as far as it can be checked without a GPU: every name is
declared and exported, the defaults are the documented ones, argument errors are reported before any device work and a
refused call writes nothing, and the Python wrappers refuse misshaped arrays before the library is called.  The checks
that read the limit arrays need the robot's dof, hence a live robot handle, hence a device: down > up, a NaN limit and a
link out of range through the C ABI are in tests/test_gpu_ik.py (as tests/test_motion_abi.py does for its limits)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpmp2_amd import _capi, scoring
from gpmp2_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gpmp2mi_ik_solve", "gpmp2mi_ik_solve_dev", "gpmp2mi_ik_solve_seeded", "gpmp2mi_ik_solve_seeded_dev",
         "gpmp2mi_ik_goals", "gpmp2mi_ik_goals_dev"]
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def _opts(eng, **kw):
    o = _capi.IkOptsC()
    eng.lib.gpmp2mi_ik_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_entry_points_and_constants_are_declared_and_exported(eng):
    hdr = open(os.path.join(ROOT, "include", "gpmp2mi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", code), f"{n} is not declared in include/gpmp2mi.h"
        assert hasattr(eng.lib, n), f"{n} is not exported"
    assert re.search(r"\bvoid\s+gpmp2mi_ik_opts_default\s*\(", code) and hasattr(eng.lib, "gpmp2mi_ik_opts_default")
    assert re.search(r"typedef\s+struct\s+gpmp2mi_ik_opts\s*\{", code)
    assert re.search(r"#define\s+GPMP2MI_IK_MAX_ITER\s+1000\b", code)
    assert re.search(r"GPMP2MI_IK_CONVERGED\s*=\s*0\s*,\s*GPMP2MI_IK_MAX_ITER_REACHED\s*=\s*1\s*,\s*GPMP2MI_IK_INVALID\s*=\s*2", code)
    assert re.search(r"GPMP2MI_RNG_IK\s*=\s*4\b", code)
    assert (_capi.RNG_IK, _capi.IK_MAX_ITER, _capi.IK_CONVERGED, _capi.IK_MAX_ITER_REACHED, _capi.IK_INVALID) == (4, 1000, 0, 1, 2)
    section = hdr[hdr.index("---- goal configurations"):hdr.index("---- misc")]
    for word in ("Determinism", "Errors", "Memory", "Not here", "gpmp2mi_multi_plan_* twins", "No angle is wrapped"):
        assert word in section, word


def test_the_defaults_are_the_documented_ones(eng):
    o = _capi.IkOptsC(7, 7, 7.0, 7.0, 7.0, 7, 7.0, 7.0, 7.0, 7.0, E.dptr(np.ones(2)), E.dptr(np.ones(2)))
    eng.lib.gpmp2mi_ik_opts_default(C.byref(o))
    assert (o.mode, o.link, o.pos_tol, o.rot_tol, o.rot_weight, o.max_iter) == (_capi.WORKSPACE_POSE, 0, 1e-6, 1e-6, 1.0, 100)
    assert (o.lambda_initial, o.lambda_factor, o.lambda_lower, o.lambda_upper) == (1e-2, 4.0, 1e-9, 1e6)
    assert not o.pos_down and not o.pos_up
    eng.lib.gpmp2mi_ik_opts_default(None)     # a no-op


def test_argument_errors_come_before_any_device_work_and_write_nothing(eng):
    lib = eng.lib
    one = C.c_void_p(1)      # a non-null handle / device pointer that must never be looked at
    des, seeds = np.eye(4).reshape(1, 16), np.zeros((1, 2, 2))
    conf, res = np.full((1, 2, 2), 7.0), np.full((1, 2, 2), 7.0)
    it, st, ng = np.full((1, 2), 7, dtype=np.int32), np.full((1, 2), 7, dtype=np.int32), np.full(1, 7, dtype=np.int32)
    gconf, gseed = np.full((1, 4, 2), 7.0), np.full((1, 4), 7, dtype=np.int32)
    d, i = E.dptr, E.iptr
    lim = np.array([-1.0, -1.0]), np.array([1.0, 1.0])
    good = _opts(eng)
    limited = _opts(eng, pos_down=d(lim[0]), pos_up=d(lim[1]))

    def solve(r=one, o=good, G=1, poses=d(des), M=2, s=d(seeds)):
        return lib.gpmp2mi_ik_solve(r, C.byref(o) if o is not None else None, G, poses, M, s, d(conf), d(res), i(it), i(st))

    def solve_dev(r=one, o=good, G=1, poses=one, M=2, s=one):
        return lib.gpmp2mi_ik_solve_dev(r, C.byref(o) if o is not None else None, G, poses, M, s, one, one, one, one, None)

    def seeded(r=one, o=limited, G=1, poses=d(des), M=2, first=0):
        return lib.gpmp2mi_ik_solve_seeded(r, C.byref(o) if o is not None else None, G, poses, M, 5, first, d(conf), d(res),
                                           i(it), i(st))

    def seeded_dev(r=one, o=limited, poses=one, first=0):
        return lib.gpmp2mi_ik_solve_seeded_dev(r, C.byref(o) if o is not None else None, 1, poses, 2, 5, first, one, one, one,
                                               one, None)

    def goals(r=one, o=good, G=1, poses=d(des), M=2, s=d(seeds), radius=0.1, max_goals=4):
        return lib.gpmp2mi_ik_goals(r, C.byref(o) if o is not None else None, None, G, poses, M, s, 5, 0, 0.0, 0, None, None,
                                    radius, max_goals, d(conf), i(st), None, None, None, i(ng), None, None, d(gconf),
                                    i(gseed), None, None)

    def goals_dev(r=one, o=good, poses=one, s=one, radius=0.1, max_goals=4):
        return lib.gpmp2mi_ik_goals_dev(r, C.byref(o) if o is not None else None, None, 1, poses, 2, s, 5, 0, 0.0, 0, None, None,
                                        radius, max_goals, *([one] * 12), None)

    bad_opts = {
        "pos_tol 0": dict(pos_tol=0.0), "pos_tol nan": dict(pos_tol=NAN), "rot_tol < 0": dict(rot_tol=-1e-6),
        "rot_tol nan": dict(rot_tol=NAN), "rot_weight 0": dict(rot_weight=0.0), "rot_weight nan": dict(rot_weight=NAN),
        "lambda_initial 0": dict(lambda_initial=0.0), "lambda_initial nan": dict(lambda_initial=NAN),
        "lambda_factor < 0": dict(lambda_factor=-4.0), "lambda_factor nan": dict(lambda_factor=NAN),
        "lambda_lower 0": dict(lambda_lower=0.0), "lambda_lower nan": dict(lambda_lower=NAN),
        "lambda_upper 0": dict(lambda_upper=0.0), "lambda_upper nan": dict(lambda_upper=NAN),
        "lambda_lower > lambda_upper": dict(lambda_lower=10.0, lambda_upper=1.0),
        "max_iter 0": dict(max_iter=0), "max_iter 1001": dict(max_iter=_capi.IK_MAX_ITER + 1),
        "mode 3": dict(mode=3), "mode -1": dict(mode=-1),
        "pos_down alone": dict(pos_down=d(lim[0])), "pos_up alone": dict(pos_up=d(lim[1])),
    }
    calls = {
        "solve robot": lambda: solve(r=None), "solve opts": lambda: solve(o=None), "solve poses": lambda: solve(poses=None),
        "solve seeds": lambda: solve(s=None), "solve G": lambda: solve(G=-1), "solve M": lambda: solve(M=-1),
        "solve_dev robot": lambda: solve_dev(r=None), "solve_dev opts": lambda: solve_dev(o=None),
        "solve_dev poses": lambda: solve_dev(poses=None), "solve_dev seeds": lambda: solve_dev(s=None),
        "solve_dev G": lambda: solve_dev(G=-1), "solve_dev M": lambda: solve_dev(M=-1),
        "seeded robot": lambda: seeded(r=None), "seeded opts": lambda: seeded(o=None), "seeded poses": lambda: seeded(poses=None),
        "seeded G": lambda: seeded(G=-1), "seeded M": lambda: seeded(M=-1), "seeded first": lambda: seeded(first=-1),
        "seeded no limits": lambda: seeded(o=good),
        "seeded_dev robot": lambda: seeded_dev(r=None), "seeded_dev poses": lambda: seeded_dev(poses=None),
        "seeded_dev first": lambda: seeded_dev(first=-1), "seeded_dev no limits": lambda: seeded_dev(o=good),
        "goals robot": lambda: goals(r=None), "goals opts": lambda: goals(o=None), "goals poses": lambda: goals(poses=None),
        "goals G": lambda: goals(G=-1), "goals M": lambda: goals(M=-1), "goals no seeds, no limits": lambda: goals(s=None),
        "goals radius < 0": lambda: goals(radius=-1e-300), "goals radius nan": lambda: goals(radius=NAN),
        "goals max_goals 0": lambda: goals(max_goals=0), "goals max_goals 65": lambda: goals(max_goals=scoring.MAX_ALTERNATIVES + 1),
        "goals_dev robot": lambda: goals_dev(r=None), "goals_dev opts": lambda: goals_dev(o=None),
        "goals_dev poses": lambda: goals_dev(poses=None), "goals_dev radius": lambda: goals_dev(radius=NAN),
        "goals_dev max_goals": lambda: goals_dev(max_goals=0),
    }
    for what, kw in bad_opts.items():
        o = _opts(eng, **kw)
        calls[f"solve {what}"] = lambda o=o: solve(o=o)
        calls[f"solve_dev {what}"] = lambda o=o: solve_dev(o=o)
        calls[f"goals {what}"] = lambda o=o: goals(o=o)
        calls[f"goals_dev {what}"] = lambda o=o: goals_dev(o=o)
        if "alone" not in what:
            o2 = _opts(eng, pos_down=d(lim[0]), pos_up=d(lim[1]), **kw)
            calls[f"seeded {what}"] = lambda o=o2: seeded(o=o)
            calls[f"seeded_dev {what}"] = lambda o=o2: seeded_dev(o=o)
    for name, call in calls.items():
        assert call() == 1, name
        assert len(lib.gpmp2mi_last_error()) > 0, name
    # a refused call writes nothing
    for a in (conf, res, it, st, ng, gconf, gseed):
        assert (a == 7).all()


def test_python_wrappers_refuse_misshaped_arrays_before_the_library_is_called():
    class Boom:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name})")

    class Robot:
        dof, L, ptr = 7, 7, None

    eng = E.Engine.__new__(E.Engine)
    eng.lib = Boom()
    o, r = _capi.IkOptsC(), Robot()
    des, seeds = np.tile(np.eye(4), (2, 1, 1)), np.zeros((2, 5, 7))
    for bad in (np.eye(3), np.zeros((2, 4, 3)), np.zeros(16)):
        with pytest.raises(ValueError):
            eng.ik_solve(r, o, bad, seeds)
        with pytest.raises(ValueError):
            eng.ik_goals(r, o, bad, seeds=seeds)
    for bad in (np.zeros((2, 5, 6)), np.zeros((3, 5, 7)), np.zeros((5, 7)), np.zeros(7)):
        with pytest.raises(ValueError):
            eng.ik_solve(r, o, des, bad)
        with pytest.raises(ValueError):
            eng.ik_goals(r, o, des, seeds=bad)
    with pytest.raises(ValueError):
        eng.ik_solve(r, o, des)                      # neither seeds nor M
    with pytest.raises(ValueError):
        eng.ik_solve(r, o, des, M=4, first=-1)
    for kw in (dict(radius=-1.0), dict(radius=NAN), dict(max_goals=0), dict(max_goals=65), dict(near=np.zeros(6)),
               dict(near=np.full(7, NAN)), dict(weights=np.ones(6)), dict(weights=-np.ones(7))):
        with pytest.raises(ValueError):
            eng.ik_goals(r, o, des, seeds=seeds, **kw)
        with pytest.raises(ValueError):
            eng.ik_goals_dev(r, o, 2, 5, 1, seeds=1, **kw)
    with pytest.raises(ValueError):
        eng.ik_goals_dev(r, o, 1, scoring.MAX_GROUP_ROWS + 1, 1, seeds=1)
    with pytest.raises(ValueError):
        eng.goal_rows(dict(n_goals=np.zeros(1, dtype=np.int32), goal_conf=np.zeros((1, 4, 7))), 4)
    rows = eng.goal_rows(dict(n_goals=np.array([3]), goal_conf=np.arange(28.0).reshape(1, 4, 7)), 5)
    assert rows.shape == (5, 7) and np.array_equal(rows[3], rows[0]) and np.array_equal(rows[4], np.arange(7.0, 14.0))
