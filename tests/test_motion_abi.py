"""The motion limits (include/gpmp2mi.h "motion limits") as far as they can be checked without a GPU: the ABI is declared
and exported, argument errors are reported before any device work, the Python helpers refuse what the C side refuses, and
without a GPU the compute calls fail loudly.  The checks that read the limit arrays need the robot's dof, hence a live
robot handle, hence a device: a NaN entry, down > up and a rate <= 0 through the C ABI are in tests/test_gpu_motion.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpmp2_amd import _capi, scoring
from gpmp2_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_NAMES = ["gpmp2mi_motion_score_traj", "gpmp2mi_motion_score_traj_dev", "gpmp2mi_plan_motion_score",
             "gpmp2mi_plan_motion_score_dev", "gpmp2mi_plan_select_feasible", "gpmp2mi_plan_select_feasible_dev"]
INF = float("inf")


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def test_entry_points_are_declared_and_exported(eng):
    hdr = open(os.path.join(ROOT, "include", "gpmp2mi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in INT_NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr), f"{n} is not declared in include/gpmp2mi.h"
        assert hasattr(eng.lib, n), f"{n} is not exported"
    assert re.search(r"\bvoid\s+gpmp2mi_motion_limits_default\s*\(", hdr) and hasattr(eng.lib, "gpmp2mi_motion_limits_default")
    assert re.search(r"typedef\s+struct\s+gpmp2mi_motion_limits\s*\{", hdr)


def test_default_limits_are_no_limits(eng):
    lim = _capi.MotionLimitsC(E.dptr(np.ones(3)), E.dptr(np.ones(3)), E.dptr(np.ones(3)), E.dptr(np.ones(3)), 2.0)
    eng.lib.gpmp2mi_motion_limits_default(C.byref(lim))
    assert not lim.pos_down and not lim.pos_up and not lim.vel and not lim.acc and lim.point_speed == INF
    eng.lib.gpmp2mi_motion_limits_default(None)     # a no-op


def test_argument_errors_are_refused_before_any_device_work(eng):
    lib = eng.lib
    t = np.zeros((1, 3, 4))
    one = C.c_void_p(1)   # a non-null handle that must never be looked at: the argument error is reported first
    ok = _capi.MotionLimitsC(None, None, None, None, INF)
    arr = np.ones(2)

    def lim(down=None, up=None, point_speed=INF):
        return C.byref(_capi.MotionLimitsC(E.dptr(down), E.dptr(up), None, None, point_speed))
    best, n, ts = C.c_int(7), C.c_int(7), C.c_double(7.0)
    tsp = C.cast(C.byref(ts), _capi.c_double_p)
    seven = [None] * 7
    bad_limits = {"point_speed 0": lim(point_speed=0.0), "point_speed < 0": lim(point_speed=-1.0),
                  "point_speed nan": lim(point_speed=float("nan")), "down alone": lim(down=arr), "up alone": lim(up=arr),
                  "null limits": None}
    calls = {
        "traj robot": lambda: lib.gpmp2mi_motion_score_traj(None, C.byref(ok), 0.1, 0, 1, 2, E.dptr(t), *seven),
        "traj traj": lambda: lib.gpmp2mi_motion_score_traj(one, C.byref(ok), 0.1, 0, 1, 2, None, *seven),
        "traj inter_step": lambda: lib.gpmp2mi_motion_score_traj(one, C.byref(ok), 0.1, -1, 1, 2, E.dptr(t), *seven),
        "traj B": lambda: lib.gpmp2mi_motion_score_traj(one, C.byref(ok), 0.1, 0, -1, 2, E.dptr(t), *seven),
        "traj total_step": lambda: lib.gpmp2mi_motion_score_traj(one, C.byref(ok), 0.1, 0, 1, 0, E.dptr(t), *seven),
        "traj delta_t": lambda: lib.gpmp2mi_motion_score_traj(one, C.byref(ok), 0.0, 0, 1, 2, E.dptr(t), *seven),
        "traj_dev robot": lambda: lib.gpmp2mi_motion_score_traj_dev(None, C.byref(ok), 0.1, 0, 1, 2, one, *seven, None),
        "traj_dev traj": lambda: lib.gpmp2mi_motion_score_traj_dev(one, C.byref(ok), 0.1, 0, 1, 2, None, *seven, None),
        "traj_dev delta_t": lambda: lib.gpmp2mi_motion_score_traj_dev(one, C.byref(ok), float("nan"), 0, 1, 2, one, *seven, None),
        "plan_motion_score plan": lambda: lib.gpmp2mi_plan_motion_score(None, C.byref(ok), 0, *seven),
        "plan_motion_score_dev plan": lambda: lib.gpmp2mi_plan_motion_score_dev(None, C.byref(ok), 0, *seven, None),
        "select_feasible plan": lambda: lib.gpmp2mi_plan_select_feasible(None, 0, 0.0, 0, None, 0.0, C.byref(ok), 0.0, 1.0,
                                                                         C.byref(best), C.byref(n), tsp, None, None),
        "select_feasible_dev plan": lambda: lib.gpmp2mi_plan_select_feasible_dev(None, 0, 0.0, 0, None, 0.0, C.byref(ok), 0.0,
                                                                                 1.0, None, None, None, None, None, None),
        "select_feasible nan margin": lambda: lib.gpmp2mi_plan_select_feasible(
            one, 0, 0.0, 0, None, 0.0, C.byref(ok), float("nan"), 1.0, C.byref(best), C.byref(n), tsp, None, None),
        "select_feasible nan scale": lambda: lib.gpmp2mi_plan_select_feasible(
            one, 0, 0.0, 0, None, 0.0, C.byref(ok), 0.0, float("nan"), C.byref(best), C.byref(n), tsp, None, None),
        "select_feasible_dev nan scale": lambda: lib.gpmp2mi_plan_select_feasible_dev(
            one, 0, 0.0, 0, None, 0.0, C.byref(ok), 0.0, float("nan"), None, None, None, None, None, None),
    }
    for what, l in bad_limits.items():
        calls[f"traj {what}"] = lambda l=l: lib.gpmp2mi_motion_score_traj(one, l, 0.1, 0, 1, 2, E.dptr(t), *seven)
        calls[f"traj_dev {what}"] = lambda l=l: lib.gpmp2mi_motion_score_traj_dev(one, l, 0.1, 0, 1, 2, one, *seven, None)
        calls[f"plan_motion_score {what}"] = lambda l=l: lib.gpmp2mi_plan_motion_score(one, l, 0, *seven)
        calls[f"plan_motion_score_dev {what}"] = lambda l=l: lib.gpmp2mi_plan_motion_score_dev(one, l, 0, *seven, None)
        calls[f"select_feasible {what}"] = lambda l=l: lib.gpmp2mi_plan_select_feasible(
            one, 0, 0.0, 0, None, 0.0, l, 0.0, 1.0, C.byref(best), C.byref(n), tsp, None, None)
        calls[f"select_feasible_dev {what}"] = lambda l=l: lib.gpmp2mi_plan_select_feasible_dev(
            one, 0, 0.0, 0, None, 0.0, l, 0.0, 1.0, None, None, None, None, None, None)
    for name, call in calls.items():
        assert call() == 1, name
        assert len(lib.gpmp2mi_last_error()) > 0, name
    assert (best.value, n.value, ts.value) == (7, 7, 7.0)      # a refused call writes nothing


def test_python_helpers_refuse_what_the_c_side_refuses():
    good = E.MotionLimits(3, pos_down=[-1, -INF, -2], pos_up=[1, 2, INF], vel=2.0, acc=[1, INF, 3], point_speed=1.5)
    assert good.vel.tolist() == [2.0, 2.0, 2.0] and good.c.point_speed == 1.5 and good.pos_down[1] == -INF
    free = E.MotionLimits(3)
    assert free.pos_down is None and free.vel is None and not free.c.pos_down and free.c.point_speed == INF
    nan = float("nan")
    for bad in (dict(pos_down=[-1, 0, 0]), dict(pos_up=[1, 1, 1]), dict(pos_down=[0, 0, 2], pos_up=[1, 1, 1]),
                dict(pos_down=[0, nan, 0], pos_up=[1, 1, 1]), dict(pos_down=[0, 0, 0], pos_up=[1, 1, nan]),
                dict(vel=[1, 0, 1]), dict(vel=[1, -2, 1]), dict(vel=[1, nan, 1]), dict(acc=0.0), dict(acc=[1, 1]),
                dict(acc=[[1, 1, 1]]), dict(point_speed=0.0), dict(point_speed=-1.0), dict(point_speed=nan)):
        with pytest.raises(ValueError):
            E.MotionLimits(3, **bad)
    with pytest.raises(ValueError):
        good.ref(7)

    class Boom:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name})")

    class Handle:
        ptr, dof = None, 3

    eng = E.Engine.__new__(E.Engine)
    eng.lib = Boom()
    r = Handle()
    ok = np.zeros((2, 5, 6))
    for bad in (np.zeros((2, 5, 5)), np.zeros((2, 5)), np.zeros((2, 1, 6))):
        with pytest.raises(ValueError):
            eng.motion_score_traj(r, good, 0.1, 2, bad)
    with pytest.raises(ValueError):
        eng.motion_score_traj(r, good, 0.1, -1, ok)
    with pytest.raises(ValueError):
        eng.motion_score_traj(r, good, 0.0, 1, ok)
    with pytest.raises(ValueError):
        eng.motion_score_traj(r, E.MotionLimits(7), 0.1, 1, ok)
    for out in ({"vel_ratio": np.zeros(3)}, {"worst": np.zeros((2, 4, 2))}, {"worst": np.zeros((2, 2), dtype=np.int32)},
                {"invalid": np.zeros(2)}, {"dense_cost": np.zeros(2)}):
        with pytest.raises(ValueError):
            eng.motion_score_traj(r, good, 0.1, 1, ok, out=out)
    pl = E.Plan.__new__(E.Plan)
    pl.eng, pl.B, pl.N, pl.D = eng, 2, 4, 3
    with pytest.raises(ValueError):
        pl.motion_score(good, -1)
    with pytest.raises(ValueError):
        pl.motion_score(good, 1, out={"time_scale": np.zeros(5)})
    with pytest.raises(ValueError):
        pl.motion_score(E.MotionLimits(7), 1)
    for kw in (dict(required_pos_margin=nan), dict(max_time_scale=nan)):
        with pytest.raises(ValueError):
            pl.select_feasible(1, good, **kw)
        with pytest.raises(ValueError):
            pl.select_feasible_dev(1, good, **kw)
    with pytest.raises(ValueError):
        pl.select_feasible(-2, good)
    assert scoring.motion_outputs(2)["worst"].shape == (2, 4, 2)


def test_without_a_gpu_the_compute_calls_fail_loudly(eng):
    """every compute call of this section starts from a robot handle or a plan, and neither exists without a device:
    the way to them raises "no usable GPU" instead of handing out something that computes elsewhere"""
    if eng.device_count() > 0:
        return          # only observable without a GPU; with one, tests/test_gpu_motion.py runs the calls
    import gpmp2_amd
    with pytest.raises(E.Gpmp2miError) as ei:
        r = eng.robot(gpmp2_amd.generateArm("WAMArm"))
        eng.motion_score_traj(r, E.MotionLimits(7, vel=2.0), 0.1, 1, np.zeros((1, 3, 14)))
    assert ei.value.code == 2
