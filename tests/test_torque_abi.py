"""Torque limits (include/gpmp2mi.h "torque limits") as far as they can be checked without a GPU: the ABI is declared,
exported and bound, argument errors are reported before any device work through pointers that are never read, the Python
helpers refuse what the C side refuses before the library is called, the rule of the selection on hand cases, and
without a GPU the compute calls answer GPMP2MI_ERR_NO_DEVICE.  The rules that read a live robot handle (the description's
values, the unsupported kinds, a handle made for another robot) are in tests/test_gpu_torque.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpmp2_amd import _capi, scoring
from gpmp2_amd import dynamics as tables
from gpmp2_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_NAMES = ["gpmp2mi_dynamics_create", "gpmp2mi_torque_score_traj", "gpmp2mi_torque_score_traj_dev",
             "gpmp2mi_plan_torque_score", "gpmp2mi_plan_torque_score_dev", "gpmp2mi_plan_select_dynamic",
             "gpmp2mi_plan_select_dynamic_dev"]
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def test_entry_points_are_declared_exported_and_bound(eng):
    hdr = open(os.path.join(ROOT, "include", "gpmp2mi.h")).read()
    assert "torque limits:" in hdr and "SAMPLED, NOT BOUNDED" in hdr
    assert "torque_ratio <= 1 <=> torque_time_scale <= 1" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in INT_NAMES:
        m = re.search(r"\bint\s+" + n + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{n} is not declared in include/gpmp2mi.h"
        assert hasattr(eng.lib, n), f"{n} is not exported"
        args = getattr(eng.lib, n).argtypes
        assert args is not None, f"{n} has no argtypes (_capi.declare_torque)"
        assert len(args) == m.group(1).count(",") + 1, f"{n}: the binding and the header disagree on the argument count"
    for n in ("gpmp2mi_dynamics_desc_default", "gpmp2mi_dynamics_destroy"):
        assert re.search(r"\bvoid\s+" + n + r"\s*\(", hdr) and hasattr(eng.lib, n)
    fields = re.search(r"typedef struct gpmp2mi_dynamics_desc \{(.*?)\}", hdr, flags=re.S).group(1)
    assert [f[0] for f in _capi.DynamicsDescC._fields_] == re.findall(r"(\w+)(?:\[3\])?;", fields)
    d = _capi.DynamicsDescC()
    d.gravity[2], d.mass = 1.0, E.dptr(np.ones(1))
    eng.lib.gpmp2mi_dynamics_desc_default(C.byref(d))
    assert list(d.gravity) == [0.0, 0.0, -9.81] and not d.mass and not d.torque
    eng.lib.gpmp2mi_dynamics_desc_default(None)
    eng.lib.gpmp2mi_dynamics_destroy(None)          # NULL: no-op


def test_argument_errors_are_refused_before_any_device_work(eng):
    lib = eng.lib
    t = np.zeros((1, 3, 4))
    one = C.c_void_p(1)   # a non-null handle that must never be looked at: the argument error is reported first
    ok = _capi.MotionLimitsC(None, None, None, None, INF)
    arr = np.ones(2)
    out = dict(a=np.full(1, 7.0), b=np.full(1, 7.0), c=np.full(1, 7.0), w=np.full((1, 3, 2), 7, dtype=np.int32),
               i=np.full(1, 7, dtype=np.int32), tau=np.full((1, 3, 2), 7.0))
    o6 = (E.dptr(out["a"]), E.dptr(out["b"]), E.dptr(out["c"]), E.iptr(out["w"]), E.iptr(out["i"]), E.dptr(out["tau"]))
    best, n, ts = C.c_int(7), C.c_int(7), C.c_double(7.0)
    tsp = C.cast(C.byref(ts), _capi.c_double_p)
    desc, made = _capi.DynamicsDescC(), C.c_void_p(7)
    m = np.ones(1)

    def lim(down=None, up=None, point_speed=INF):
        return C.byref(_capi.MotionLimitsC(E.dptr(down), E.dptr(up), None, None, point_speed))

    def traj(r=one, y=one, dt=0.1, J=0, B=1, N=2, tr=E.dptr(t)):
        return lambda: lib.gpmp2mi_torque_score_traj(r, y, dt, J, B, N, tr, *o6)

    def traj_dev(r=one, y=one, dt=0.1, J=0, B=1, N=2, tr=one):
        return lambda: lib.gpmp2mi_torque_score_traj_dev(r, y, dt, J, B, N, tr, *([None] * 6), None)

    def sel(p=one, y=one, l=C.byref(ok), rpm=0.0, mts=1.0):
        return lambda: lib.gpmp2mi_plan_select_dynamic(p, 0, 0.0, 0, None, 0.0, l, rpm, mts, y, C.byref(best), C.byref(n),
                                                       tsp, None, None, None)

    def sel_dev(p=one, y=one, l=C.byref(ok), rpm=0.0, mts=1.0):
        return lambda: lib.gpmp2mi_plan_select_dynamic_dev(p, 0, 0.0, 0, None, 0.0, l, rpm, mts, y, *([None] * 6), None)

    calls = {
        "create robot": lambda: lib.gpmp2mi_dynamics_create(None, C.byref(desc), C.byref(made)),
        "create desc": lambda: lib.gpmp2mi_dynamics_create(one, None, C.byref(made)),
        "create out": lambda: lib.gpmp2mi_dynamics_create(one, C.byref(desc), None),
        "create null arrays": lambda: lib.gpmp2mi_dynamics_create(one, C.byref(desc), C.byref(made)),
        "create null com": lambda: lib.gpmp2mi_dynamics_create(
            one, C.byref(_capi.DynamicsDescC(E.dptr(m), None, E.dptr(m), (C.c_double * 3)(), None)), C.byref(made)),
        "traj robot": traj(r=None), "traj dynamics": traj(y=None), "traj traj": traj(tr=None),
        "traj_dev robot": traj_dev(r=None), "traj_dev dynamics": traj_dev(y=None), "traj_dev traj": traj_dev(tr=None),
        "plan plan": lambda: lib.gpmp2mi_plan_torque_score(None, one, 0, *o6),
        "plan dynamics": lambda: lib.gpmp2mi_plan_torque_score(one, None, 0, *o6),
        "plan_dev plan": lambda: lib.gpmp2mi_plan_torque_score_dev(None, one, 0, *([None] * 6), None),
        "plan_dev dynamics": lambda: lib.gpmp2mi_plan_torque_score_dev(one, None, 0, *([None] * 6), None),
        "select plan": sel(p=None), "select dynamics": sel(y=None), "select_dev plan": sel_dev(p=None),
        "select_dev dynamics": sel_dev(y=None), "select nan margin": sel(rpm=NAN), "select nan scale": sel(mts=NAN),
        "select_dev nan scale": sel_dev(mts=NAN),
    }
    bad_limits = {"point_speed 0": lim(point_speed=0.0), "point_speed nan": lim(point_speed=NAN), "down alone": lim(down=arr),
                  "up alone": lim(up=arr), "null limits": None}
    for what, l in bad_limits.items():
        calls[f"select {what}"] = sel(l=l)
        calls[f"select_dev {what}"] = sel_dev(l=l)
    for name, call in calls.items():
        assert call() == 1, name
        assert len(lib.gpmp2mi_last_error()) > 0, name
    assert (best.value, n.value, ts.value) == (7, 7, 7.0)      # a refused call writes nothing
    for name, x in out.items():
        assert (x == 7).all(), name
    assert made.value is None or made.value == 7               # never a handle


def test_python_helpers_refuse_what_the_c_side_refuses():
    t = tables.illustrative_wam()
    good = dict(mass=t["mass"], com=t["com"], inertia=t["inertia"])
    m, c, i, g, tq = scoring.dynamics_table(7, 7, torque=50.0, **good)
    assert tq.shape == (7,) and (tq == 50.0).all() and list(g) == [0.0, 0.0, -9.81] and i.shape == (7, 6)
    assert scoring.dynamics_table(7, 7, torque=None, **good)[4] is None
    assert np.isposinf(scoring.dynamics_table(7, 7, torque=[1, INF, 1, 1, 1, 1, 1], **good)[4][1])
    neg_mass, nan_com, neg_diag = t["mass"].copy(), t["com"].copy(), t["inertia"].copy()
    neg_mass[3], nan_com[2, 1], neg_diag[4, 2] = -1.0, NAN, -1e-3
    for kw in (dict(mass=neg_mass), dict(com=nan_com), dict(inertia=neg_diag), dict(mass=t["mass"][:6]),
               dict(com=t["com"].T), dict(inertia=t["inertia"][:, :3]), dict(gravity=[0, 0]), dict(gravity=[0, NAN, 0]),
               dict(torque=0.0), dict(torque=NAN), dict(torque=[1.0] * 6), dict(torque=[1, 1, 1, -1, 1, 1, 1])):
        with pytest.raises(ValueError):
            scoring.dynamics_table(7, 7, **dict(good, **kw))
    o = scoring.torque_outputs(2, 5, 3)
    assert o["tau"].shape == (2, 5, 3) and o["worst"].shape == (2, 3, 2) and o["invalid"].dtype == np.int32
    assert scoring.torque_outputs(2, 5, 3, tau=False)["tau"] is None
    for bad in ({"tau": np.zeros((2, 5, 4))}, {"worst": np.zeros((2, 3, 2))}, {"time_scale": np.zeros(2)}):
        with pytest.raises(ValueError):
            scoring.torque_outputs(2, 5, 3, bad)

    class Boom:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name})")

    class Handle:
        ptr, dof, L = None, 7, 7

    eng = E.Engine.__new__(E.Engine)
    eng.lib = Boom()
    r, y = Handle(), Handle()
    with pytest.raises(ValueError):
        eng.dynamics(r, neg_mass, t["com"], t["inertia"])
    with pytest.raises(ValueError):
        eng.dynamics(r, t["mass"], t["com"], t["inertia"], torque=[1.0, 2.0])
    ok = np.zeros((2, 5, 14))
    for bad in (np.zeros((2, 5, 13)), np.zeros((2, 5)), np.zeros((2, 1, 14))):
        with pytest.raises(ValueError):
            eng.torque_score_traj(r, y, 0.1, 2, bad)
    for kw in (dict(inter_step=-1), dict(delta_t=0.0), dict(out={"tau": np.zeros((2, 5, 7))}),
               dict(out={"invalid": np.zeros(2)})):
        with pytest.raises(ValueError):
            eng.torque_score_traj(r, y, **dict(dict(delta_t=0.1, inter_step=1, traj=ok), **kw))
    pl = E.Plan.__new__(E.Plan)
    pl.eng, pl.B, pl.N, pl.D = eng, 2, 4, 7
    lim = E.MotionLimits(7, vel=2.0)
    for call in (pl.torque_score, pl.torque_score_dev):
        with pytest.raises(ValueError):
            call(y, -1)
    with pytest.raises(ValueError):
        pl.torque_score(y, 1, out={"tau": np.zeros((2, 5, 7))})
    for call in (pl.select_dynamic, pl.select_dynamic_dev):
        for kw in (dict(required_pos_margin=NAN), dict(max_time_scale=NAN)):
            with pytest.raises(ValueError):
                call(1, lim, y, **kw)
        with pytest.raises(ValueError):
            call(-2, lim, y)
        with pytest.raises(ValueError):
            call(1, E.MotionLimits(3), y)


def test_dynamic_rule_on_hand_cases():
    fe = np.array([3.0, 1.0, 1.0, 0.5, np.nan])
    st = np.array([0, 0, 0, 3, 0])
    clr, oor = np.full(5, 0.1), np.zeros(5, dtype=np.int32)
    ts, tts = np.array([0.5, 2.0, 0.9, 0.1, 0.1]), np.array([0.8, 0.5, 1.5, 0.1, 0.1])
    rule = scoring.dynamic_rule
    kw = dict(time_scale=ts, torque_time_scale=tts)
    # no threshold: the rule of select_rule (row 3 is not SPD, row 4 not finite; the tie goes to the lower row)
    assert rule(fe, st, clr, oor, **kw) == scoring.select_rule(fe, st, clr, oor) == (1, 3)
    assert rule(fe, st, clr, oor, max_time_scale=2.0, **kw) == (1, 3)           # <=, not <; the larger of the two counts
    assert rule(fe, st, clr, oor, max_time_scale=1.9, **kw) == (2, 2)
    assert rule(fe, st, clr, oor, max_time_scale=1.0, **kw) == (0, 1)
    assert rule(fe, st, clr, oor, max_time_scale=0.7, **kw) == (-1, 0)
    assert rule(fe, st, clr, oor, time_scale=ts, torque_time_scale=np.array([0.1, INF, 0.1, 0.1, 0.1]),
                max_time_scale=1e300) == (2, 2)
    assert rule(fe, st, clr, oor, torque_invalid=np.array([0, 1, 1, 0, 0]), **kw) == (0, 1)
    assert rule(fe, st, clr, oor, motion_invalid=np.array([0, 1, 0, 0, 0]), **kw) == (2, 2)
    assert rule(fe, st, clr, oor, pos_margin=np.array([0.1, -0.1, 0.1, 0.1, 0.1]), **kw) == (2, 2)
    assert rule(fe, st, clr, oor, required_clearance=0.2, **kw) == (-1, 0)
    # without the torque side it is feasible_rule
    assert rule(fe, st, clr, oor, time_scale=ts, max_time_scale=1.0) == \
        scoring.feasible_rule(fe, st, clr, oor, time_scale=ts, max_time_scale=1.0)


def test_without_a_gpu_the_compute_calls_answer_no_device(eng):
    """every call of this section starts from a robot handle, and the way to that raises no-device rather than
    computing elsewhere"""
    if eng.device_count() > 0:
        return          # only observable without a GPU; with one, tests/test_gpu_torque.py runs the calls
    import gpmp2_amd
    t = tables.illustrative_wam()
    with pytest.raises(E.Gpmp2miError) as ei:
        r = eng.robot(gpmp2_amd.generateArm("WAMArm"))
        y = eng.dynamics(r, t["mass"], t["com"], t["inertia"], torque=t["torque"])
        eng.torque_score_traj(r, y, 0.1, 1, np.zeros((1, 3, 14)))
    assert ei.value.code == 2
