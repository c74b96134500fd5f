"""Re-timing (include/gpmp2mi.h "re-timing") as far as it can be checked without a GPU: the ABI is declared, exported and
bound, argument errors are reported before any device work through pointers that are never read, the Python helpers
refuse what the C side refuses, and without a GPU the compute calls answer GPMP2MI_ERR_NO_DEVICE.  The refusal of the
Pose2 kinds reads the kind of a live robot handle, hence needs a device: it is in tests/test_gpu_retime.py, with its
message."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpmp2_amd import _capi, scoring
from gpmp2_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_NAMES = ["gpmp2mi_retime_path", "gpmp2mi_retime_path_dev", "gpmp2mi_retime_traj", "gpmp2mi_retime_traj_dev",
             "gpmp2mi_plan_retime", "gpmp2mi_plan_retime_dev", "gpmp2mi_plan_select_retimed",
             "gpmp2mi_plan_select_retimed_dev"]
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def test_entry_points_are_declared_exported_and_bound(eng):
    hdr = open(os.path.join(ROOT, "include", "gpmp2mi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in INT_NAMES:
        m = re.search(r"\bint\s+" + n + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{n} is not declared in include/gpmp2mi.h"
        assert hasattr(eng.lib, n), f"{n} is not exported"
        args = getattr(eng.lib, n).argtypes
        assert args is not None, f"{n} has no argtypes (_capi.declare_retime)"
        assert len(args) == m.group(1).count(",") + 1, f"{n}: the binding and the header disagree on the argument count"
    for k, name in enumerate(("OK", "BOUNDARY", "EMPTY", "INVALID")):
        assert re.search(rf"GPMP2MI_RETIME_{name}\s*=\s*{k}\b", hdr)
    assert (scoring.RETIME_OK, scoring.RETIME_BOUNDARY, scoring.RETIME_EMPTY, scoring.RETIME_INVALID) == (0, 1, 2, 3)
    rule = open(os.path.join(ROOT, "gpmp2_amd", "csrc", "retime_rule.h")).read()
    assert "RETIME_OK = 0, RETIME_BOUNDARY = 1, RETIME_EMPTY = 2, RETIME_INVALID = 3" in rule


def test_argument_errors_are_refused_before_any_device_work(eng):
    lib = eng.lib
    t = np.zeros((1, 3, 4))
    one = C.c_void_p(1)   # a non-null handle that must never be looked at: the argument error is reported first
    ok = _capi.MotionLimitsC(None, None, None, None, INF)
    arr = np.ones(2)
    q, cap = np.zeros((1, 3, 2)), np.full((1, 3), INF)
    q_, c_, t_ = E.dptr(q), E.dptr(cap), E.dptr(t)
    out = dict(sdot=np.full((1, 3), 7.0), u=np.full((1, 3), 7.0), stamps=np.full((1, 3), 7.0), duration=np.full(1, 7.0),
               status=np.full(1, 7, dtype=np.int32), achieved=np.full((1, 4), 7.0))
    o6 = (E.dptr(out["sdot"]), E.dptr(out["u"]), E.dptr(out["stamps"]), E.dptr(out["duration"]), E.iptr(out["status"]),
          E.dptr(out["achieved"]))
    seven = [None] * 7
    best, n, dur = C.c_int(7), C.c_int(7), C.c_double(7.0)
    durp = C.cast(C.byref(dur), _capi.c_double_p)

    def lim(down=None, up=None, point_speed=INF):
        return C.byref(_capi.MotionLimitsC(E.dptr(down), E.dptr(up), None, None, point_speed))

    def path(B=1, Md=3, dof=2, qd=q_, ql=q_, qr=q_, cp=c_, acc=None, h=0.1, rates=(1.0, -1.0, -1.0)):
        return lambda: lib.gpmp2mi_retime_path(B, Md, dof, qd, ql, qr, cp, E.dptr(acc), h, *rates, *o6)

    def path_dev(sdot=one, u=one, stamps=one, ws=one, Md=3, rates=(1.0, -1.0, -1.0)):
        return lambda: lib.gpmp2mi_retime_path_dev(1, Md, 2, one, one, one, one, None, 0.1, *rates, sdot, u, stamps, None,
                                                   None, None, ws, None)

    def traj(r=one, l=C.byref(ok), dt=0.1, J=0, B=1, N=2, tr=t_, rates=(1.0, -1.0, -1.0)):
        return lambda: lib.gpmp2mi_retime_traj(r, l, dt, J, B, N, tr, *rates, *seven)

    def traj_dev(r=one, l=C.byref(ok), dt=0.1, J=0, B=1, N=2, tr=one, rates=(1.0, -1.0, -1.0)):
        return lambda: lib.gpmp2mi_retime_traj_dev(r, l, dt, J, B, N, tr, *rates, *seven, None)

    def plan(p=one, l=C.byref(ok), rates=(1.0, -1.0, -1.0)):
        return lambda: lib.gpmp2mi_plan_retime(p, l, 0, *rates, *seven)

    def plan_dev(p=one, l=C.byref(ok), rates=(1.0, -1.0, -1.0)):
        return lambda: lib.gpmp2mi_plan_retime_dev(p, l, 0, *rates, *seven, None)

    def sel(p=one, l=C.byref(ok), rpm=0.0, rates=(1.0, -1.0, -1.0), md=INF):
        return lambda: lib.gpmp2mi_plan_select_retimed(p, 0, 0.0, 0, None, 0.0, l, rpm, *rates, md, C.byref(best),
                                                       C.byref(n), durp, None, None, None)

    def sel_dev(p=one, l=C.byref(ok), rpm=0.0, rates=(1.0, -1.0, -1.0), md=INF):
        return lambda: lib.gpmp2mi_plan_select_retimed_dev(p, 0, 0.0, 0, None, 0.0, l, rpm, *rates, md, None, None, None,
                                                           None, None, None, None)

    calls = {
        "path qd": path(qd=None), "path qdd_left": path(ql=None), "path qdd_right": path(qr=None), "path cap": path(cp=None),
        "path B": path(B=-1), "path Md": path(Md=1), "path dof 0": path(dof=0), "path dof 19": path(dof=19),
        "path h 0": path(h=0.0), "path h nan": path(h=NAN), "path h inf": path(h=INF),
        "path acc 0": path(acc=np.array([1.0, 0.0])), "path acc nan": path(acc=np.array([NAN, 1.0])),
        "path_dev sdot": path_dev(sdot=None), "path_dev u": path_dev(u=None), "path_dev stamps": path_dev(stamps=None),
        "path_dev workspace": path_dev(ws=None), "path_dev Md": path_dev(Md=0),
        "traj robot": traj(r=None), "traj traj": traj(tr=None), "traj inter_step": traj(J=-1), "traj B": traj(B=-1),
        "traj total_step": traj(N=0), "traj delta_t": traj(dt=0.0),
        "traj_dev robot": traj_dev(r=None), "traj_dev traj": traj_dev(tr=None), "traj_dev delta_t": traj_dev(dt=NAN),
        "plan plan": plan(p=None), "plan_dev plan": plan_dev(p=None), "select plan": sel(p=None),
        "select_dev plan": sel_dev(p=None), "select nan margin": sel(rpm=NAN), "select nan duration": sel(md=NAN),
        "select_dev nan duration": sel_dev(md=NAN),
    }
    bad_rates = {"max_rate 0": (0.0, -1.0, -1.0), "max_rate < 0": (-1.0, -1.0, -1.0), "max_rate inf": (INF, -1.0, -1.0),
                 "max_rate nan": (NAN, -1.0, -1.0), "rate_start nan": (1.0, NAN, -1.0), "rate_end nan": (1.0, -1.0, NAN)}
    for what, r in bad_rates.items():
        for form, make in (("path", path), ("path_dev", path_dev), ("traj", traj), ("traj_dev", traj_dev), ("plan", plan),
                           ("plan_dev", plan_dev), ("select", sel), ("select_dev", sel_dev)):
            calls[f"{form} {what}"] = make(rates=r)
    bad_limits = {"point_speed 0": lim(point_speed=0.0), "point_speed nan": lim(point_speed=NAN), "down alone": lim(down=arr),
                  "up alone": lim(up=arr), "null limits": None}
    for what, l in bad_limits.items():
        for form, make in (("traj", traj), ("traj_dev", traj_dev), ("plan", plan), ("plan_dev", plan_dev), ("select", sel),
                           ("select_dev", sel_dev)):
            calls[f"{form} {what}"] = make(l=l)
    for name, call in calls.items():
        assert call() == 1, name
        assert len(lib.gpmp2mi_last_error()) > 0, name
    assert (best.value, n.value, dur.value) == (7, 7, 7.0)      # a refused call writes nothing
    for name, x in out.items():
        assert (x == 7).all(), name
    assert lib.gpmp2mi_retime_path(1, 3, 2, q_, q_, q_, c_, None, 0.1, 0.0, -1.0, -1.0, *o6) == 1
    assert b"max_rate" in lib.gpmp2mi_last_error()


def test_python_helpers_refuse_what_the_c_side_refuses():
    assert scoring.retime_rates() == (1.0, -1.0, -1.0)
    assert scoring.retime_rates(2.0, 0.0, 0.5) == (2.0, 0.0, 0.5)
    for bad in (dict(max_rate=0.0), dict(max_rate=-1.0), dict(max_rate=INF), dict(max_rate=NAN), dict(rate_start=NAN),
                dict(rate_end=NAN), dict(rate_start=-0.5), dict(rate_end=-1.0)):
        with pytest.raises(ValueError):
            scoring.retime_rates(**bad)
    o = scoring.retime_outputs(2, 5, 3)
    assert o["sdot"].shape == (2, 5) and o["achieved"].shape == (2, 4) and o["dense_retimed"].shape == (2, 5, 6)
    assert o["status"].dtype == np.int32 and "dense_retimed" not in scoring.retime_outputs(2, 5)

    class Boom:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name})")

    class Handle:
        ptr, dof = None, 3

    eng = E.Engine.__new__(E.Engine)
    eng.lib = Boom()
    r, good = Handle(), E.MotionLimits(3, vel=2.0, acc=[1, INF, 3], point_speed=1.5)
    ok = np.zeros((2, 5, 6))
    for bad in (np.zeros((2, 5, 5)), np.zeros((2, 5)), np.zeros((2, 1, 6))):
        with pytest.raises(ValueError):
            eng.retime_traj(r, good, 0.1, 2, bad)
    for kw in (dict(inter_step=-1), dict(delta_t=0.0), dict(max_rate=0.0), dict(rate_end=NAN), dict(limits=E.MotionLimits(7)),
               dict(out={"sdot": np.zeros((2, 4))}), dict(out={"status": np.zeros(2)}), dict(out={"time_scale": np.zeros(2)})):
        args = dict(dict(limits=good, delta_t=0.1, inter_step=1), **kw)
        with pytest.raises(ValueError):
            eng.retime_traj(r, traj=ok, **args)
    q, cap = np.zeros((2, 4, 3)), np.ones((2, 4))
    for kw in (dict(qd=np.zeros((2, 1, 3))), dict(cap=np.ones((2, 5))), dict(acc=[1.0, 0.0, 1.0]), dict(acc=[1.0, 1.0]),
               dict(h=0.0), dict(h=INF), dict(max_rate=NAN), dict(out={"dense_retimed": np.zeros((2, 4, 6))})):
        args = dict(dict(qd=q, qdd_left=q, qdd_right=q, cap=cap, acc=None, h=0.1), **kw)
        with pytest.raises(ValueError):
            eng.retime_path(**args)
    pl = E.Plan.__new__(E.Plan)
    pl.eng, pl.B, pl.N, pl.D = eng, 2, 4, 3
    for call in (pl.retime, pl.retime_dev):
        with pytest.raises(ValueError):
            call(good, -1)
        with pytest.raises(ValueError):
            call(good, 1, max_rate=INF)
        with pytest.raises(ValueError):
            call(E.MotionLimits(7), 1)
    with pytest.raises(ValueError):
        pl.retime(good, 1, out={"stamps": np.zeros((2, 4))})
    for call in (pl.select_retimed, pl.select_retimed_dev):
        for kw in (dict(required_pos_margin=NAN), dict(max_duration=NAN), dict(max_rate=0.0), dict(rate_start=-1.0)):
            with pytest.raises(ValueError):
                call(1, good, **kw)
        with pytest.raises(ValueError):
            call(-2, good)


def test_retimed_rule_on_hand_cases():
    fe = np.array([3.0, 1.0, 1.0, 0.5, np.nan])
    st = np.array([0, 0, 0, 3, 0])
    clr, oor = np.full(5, 0.1), np.zeros(5, dtype=np.int32)
    rs, dur = np.zeros(5, dtype=np.int32), np.array([2.0, 3.0, 2.5, 1.0, 1.0])
    rule = scoring.retimed_rule
    # every row re-times: the rule of select_rule (row 3 is not SPD, row 4 not finite; the tie goes to the lower row)
    assert rule(fe, st, clr, oor, retime_status=rs, duration=dur) == scoring.select_rule(fe, st, clr, oor) == (1, 3)
    assert rule(fe, st, clr, oor, retime_status=rs, duration=dur, max_duration=2.5) == (2, 2)      # <=, not <
    assert rule(fe, st, clr, oor, retime_status=rs, duration=dur, max_duration=2.0) == (0, 1)
    assert rule(fe, st, clr, oor, retime_status=rs, duration=dur, max_duration=1.5) == (-1, 0)
    assert rule(fe, st, clr, oor, retime_status=np.array([0, 2, 0, 0, 0]), duration=dur) == (2, 2)
    assert rule(fe, st, clr, oor, retime_status=np.array([0, 1, 3, 0, 0]), duration=dur) == (0, 1)
    assert rule(fe, st, clr, oor, retime_status=rs, duration=np.full(5, np.nan)) == (-1, 0)
    assert rule(fe, st, clr, oor, retime_status=rs, duration=dur, pos_margin=np.array([0.1, -0.1, 0.1, 0.1, 0.1])) == (2, 2)
    assert rule(fe, st, clr, oor, retime_status=rs, duration=dur, motion_invalid=np.array([0, 1, 1, 0, 0])) == (0, 1)
    assert rule(fe, st, clr, oor, retime_status=rs, duration=dur, required_clearance=0.2) == (-1, 0)


def test_without_a_gpu_the_compute_calls_answer_no_device(eng):
    """gpmp2mi_retime_path starts from no handle: it is the one call of this section that can be made without a device,
    and it answers GPMP2MI_ERR_NO_DEVICE rather than computing elsewhere; the others start from a robot handle or a
    plan, and the way to those raises the same"""
    if eng.device_count() > 0:
        return          # only observable without a GPU; with one, tests/test_gpu_retime.py runs the calls
    q, cap = np.zeros((1, 3, 2)), np.full((1, 3), INF)
    with pytest.raises(E.Gpmp2miError) as ei:
        eng.retime_path(q, q, q, cap, None, 0.1)
    assert ei.value.code == 2
    import gpmp2_amd
    with pytest.raises(E.Gpmp2miError) as ei:
        r = eng.robot(gpmp2_amd.generateArm("WAMArm"))
        eng.retime_traj(r, E.MotionLimits(7, vel=2.0), 0.1, 1, np.zeros((1, 3, 14)))
    assert ei.value.code == 2
