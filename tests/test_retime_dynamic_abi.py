"""Re-timing under torque limits (include/gpmp2mi.h) as far as it can be checked without a GPU: the ABI is declared,
exported and bound, argument errors are reported before any device work through pointers that are never read, the Python
helpers refuse what the C side refuses before the library is called, and without a GPU the compute calls answer
GPMP2MI_ERR_NO_DEVICE.  The rules that read a live handle (the unsupported kinds, a dynamics handle made for another
robot) are in tests/test_gpu_retime_dynamic.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpmp2_amd import _capi, scoring, stages
from gpmp2_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_NAMES = ["gpmp2mi_retime_path_affine", "gpmp2mi_retime_path_affine_dev", "gpmp2mi_retime_dynamic_traj",
             "gpmp2mi_retime_dynamic_traj_dev", "gpmp2mi_plan_retime_dynamic", "gpmp2mi_plan_retime_dynamic_dev",
             "gpmp2mi_plan_select_retimed_dynamic", "gpmp2mi_plan_select_retimed_dynamic_dev"]
INF, NAN = float("inf"), float("nan")
RATES = (1.0, -1.0, -1.0)


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def test_entry_points_are_declared_exported_and_bound(eng):
    text = open(os.path.join(ROOT, "include", "gpmp2mi.h")).read()
    assert "re-timing under torque limits:" in text and "SAMPLED, NOT BOUNDED" in text
    assert "the rule knows symmetric rows" not in text and "the torques of an already re-timed row" not in text
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in INT_NAMES:
        m = re.search(r"\bint\s+" + n + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{n} is not declared in include/gpmp2mi.h"
        assert hasattr(eng.lib, n), f"{n} is not exported"
        args = getattr(eng.lib, n).argtypes
        assert args is not None, f"{n} has no argtypes (_capi.declare_retime_dynamic)"
        assert len(args) == m.group(1).count(",") + 1, f"{n}: the binding and the header disagree on the argument count"
        outs = stages.RETIME_AFFINE if "path" in n else stages.RETIME_DYNAMIC
        if "select" not in n:          # the entry point ends in the stage's outputs, in order
            tail = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
            tail = [a for a in tail if a not in ("workspace", "stream")]
            assert tail[-len(outs.outputs):] == list(stages.names(outs)), n
    for k, name in enumerate(("OK", "BOUNDARY", "EMPTY", "INVALID", "STATIC")):
        assert re.search(rf"GPMP2MI_RETIME_{name}\s*=\s*{k}\b", hdr)
    assert scoring.RETIME_STATIC == 4
    rule = open(os.path.join(ROOT, "gpmp2_amd", "csrc", "retime_affine_rule.h")).read()
    assert "RETIME_STATIC = 4" in rule and "RETIME_MAX_EXTRA = 8" in rule
    assert stages.RETIME_DYNAMIC.absent == {"tau_retimed": "null", "coef": "null"} and not stages.RETIME_AFFINE.absent
    assert list(stages.STAGES) == ["score", "self", "moving", "path", "motion", "torque", "retime"]


def test_argument_errors_are_refused_before_any_device_work(eng):
    lib = eng.lib
    t = np.zeros((1, 3, 4))
    one = C.c_void_p(1)   # a non-null handle that must never be looked at: the argument error is reported first
    ok = _capi.MotionLimitsC(None, None, None, None, INF)
    arr = np.ones(2)
    q, cap, rows = np.zeros((1, 3, 2)), np.full((1, 3), INF), np.zeros((1, 3, 2))
    q_, c_, t_, r_ = E.dptr(q), E.dptr(cap), E.dptr(t), E.dptr(rows)
    out = dict(sdot=np.full((1, 3), 7.0), u=np.full((1, 3), 7.0), stamps=np.full((1, 3), 7.0), duration=np.full(1, 7.0),
               status=np.full(1, 7, dtype=np.int32), achieved=np.full((1, 6), 7.0))
    o6 = (E.dptr(out["sdot"]), E.dptr(out["u"]), E.dptr(out["stamps"]), E.dptr(out["duration"]), E.iptr(out["status"]),
          E.dptr(out["achieved"]))
    nine = [None] * 9
    best, n, dur = C.c_int(7), C.c_int(7), C.c_double(7.0)
    durp = C.cast(C.byref(dur), _capi.c_double_p)
    two = np.array([1.0, 2.0])

    def lim(down=None, up=None, point_speed=INF):
        return C.byref(_capi.MotionLimitsC(E.dptr(down), E.dptr(up), None, None, point_speed))

    def path(B=1, Md=3, dof=2, qd=q_, ql=q_, qr=q_, cp=c_, acc=None, R=2, cxl=r_, cxr=r_, cu=r_, off=r_, bound=two, h=0.1,
             rates=RATES):
        return lambda: lib.gpmp2mi_retime_path_affine(B, Md, dof, qd, ql, qr, cp, E.dptr(acc), R, cxl, cxr, cu, off,
                                                      E.dptr(bound), h, *rates, *o6)

    def path_dev(sdot=one, u=one, stamps=one, ws=one, Md=3, R=2, bound=two, rates=RATES):
        return lambda: lib.gpmp2mi_retime_path_affine_dev(1, Md, 2, one, one, one, one, None, R, one, one, one, one,
                                                          E.dptr(bound), 0.1, *rates, sdot, u, stamps, None, None, None, ws,
                                                          None)

    def traj(r=one, y=one, l=C.byref(ok), dt=0.1, J=0, B=1, N=2, tr=t_, rates=RATES):
        return lambda: lib.gpmp2mi_retime_dynamic_traj(r, y, l, dt, J, B, N, tr, *rates, *nine)

    def traj_dev(r=one, y=one, l=C.byref(ok), dt=0.1, J=0, B=1, N=2, tr=one, rates=RATES):
        return lambda: lib.gpmp2mi_retime_dynamic_traj_dev(r, y, l, dt, J, B, N, tr, *rates, *nine, None)

    def plan(p=one, y=one, l=C.byref(ok), rates=RATES):
        return lambda: lib.gpmp2mi_plan_retime_dynamic(p, y, l, 0, *rates, *nine)

    def plan_dev(p=one, y=one, l=C.byref(ok), rates=RATES):
        return lambda: lib.gpmp2mi_plan_retime_dynamic_dev(p, y, l, 0, *rates, *nine, None)

    def sel(p=one, y=one, l=C.byref(ok), rpm=0.0, rates=RATES, md=INF):
        return lambda: lib.gpmp2mi_plan_select_retimed_dynamic(p, 0, 0.0, 0, None, 0.0, l, rpm, *rates, md, y, C.byref(best),
                                                               C.byref(n), durp, None, None, None, None)

    def sel_dev(p=one, y=one, l=C.byref(ok), rpm=0.0, rates=RATES, md=INF):
        return lambda: lib.gpmp2mi_plan_select_retimed_dynamic_dev(p, 0, 0.0, 0, None, 0.0, l, rpm, *rates, md, y,
                                                                   *([None] * 7), None)

    calls = {
        "path qd": path(qd=None), "path qdd_left": path(ql=None), "path qdd_right": path(qr=None), "path cap": path(cp=None),
        "path B": path(B=-1), "path Md": path(Md=1), "path dof 0": path(dof=0), "path dof 19": path(dof=19),
        "path h 0": path(h=0.0), "path h nan": path(h=NAN), "path h inf": path(h=INF),
        "path acc 0": path(acc=np.array([1.0, 0.0])), "path acc nan": path(acc=np.array([NAN, 1.0])),
        "path R -1": path(R=-1), "path R 9": path(R=9), "path cx_left": path(cxl=None), "path cx_right": path(cxr=None),
        "path cu": path(cu=None), "path off": path(off=None), "path bound": path(bound=None),
        "path bound 0": path(bound=np.array([1.0, 0.0])), "path bound < 0": path(bound=np.array([-1.0, 1.0])),
        "path bound nan": path(bound=np.array([1.0, NAN])),
        "path_dev sdot": path_dev(sdot=None), "path_dev u": path_dev(u=None), "path_dev stamps": path_dev(stamps=None),
        "path_dev workspace": path_dev(ws=None), "path_dev Md": path_dev(Md=0), "path_dev R 9": path_dev(R=9),
        "path_dev bound nan": path_dev(bound=np.array([NAN, 1.0])),
        "traj robot": traj(r=None), "traj dynamics": traj(y=None), "traj traj": traj(tr=None), "traj inter_step": traj(J=-1),
        "traj B": traj(B=-1), "traj total_step": traj(N=0), "traj delta_t": traj(dt=0.0),
        "traj_dev robot": traj_dev(r=None), "traj_dev dynamics": traj_dev(y=None), "traj_dev traj": traj_dev(tr=None),
        "traj_dev delta_t": traj_dev(dt=NAN),
        "plan plan": plan(p=None), "plan dynamics": plan(y=None), "plan_dev plan": plan_dev(p=None),
        "plan_dev dynamics": plan_dev(y=None), "select plan": sel(p=None), "select dynamics": sel(y=None),
        "select_dev plan": sel_dev(p=None), "select_dev dynamics": sel_dev(y=None), "select nan margin": sel(rpm=NAN),
        "select nan duration": sel(md=NAN), "select_dev nan duration": sel_dev(md=NAN),
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
    assert path(R=9)() == 1 and b"R outside 0..8" in lib.gpmp2mi_last_error()
    assert path(bound=np.array([1.0, NAN]))() == 1 and b"bound" in lib.gpmp2mi_last_error()
    # B = 0 is fine, with or without affine rows, and needs no device
    assert path(B=0)() == 0 and path(B=0, R=0, cxl=None, cxr=None, cu=None, off=None, bound=None)() == 0


def test_python_helpers_refuse_what_the_c_side_refuses():
    o = scoring.retime_dynamic_outputs(2, 5, 3)
    assert o["sdot"].shape == (2, 5) and o["achieved"].shape == (2, 6) and o["dense_retimed"].shape == (2, 5, 6)
    assert o["tau_retimed"].shape == (2, 5, 3) and o["coef"].shape == (2, 5, 4, 3) and o["status"].dtype == np.int32
    assert list(o) == list(scoring.RETIME_DYNAMIC_NAMES)
    lean = scoring.retime_dynamic_outputs(2, 5, 3, tau=False, coef=False)
    assert lean["tau_retimed"] is None and lean["coef"] is None and list(lean) == list(o)
    assert list(scoring.retime_affine_outputs(2, 5)) == list(scoring.RETIME_DYNAMIC_NAMES[:6])
    R, cxl, cxr, cu, off, b = scoring.affine_rows(2, 4, np.zeros((2, 4, 3)), np.zeros((2, 4, 3)), np.zeros((2, 4, 3)),
                                                  np.zeros((2, 4, 3)), [1.0, INF, 2.0])
    assert R == 3 and cxl.shape == (2, 4, 3) and b.dtype == np.float64
    assert scoring.affine_rows(2, 4, None, None, None, None, None)[0] == 0
    z = np.zeros((2, 4, 2))
    for bad in (dict(bound=[1.0, 0.0]), dict(bound=[1.0, NAN]), dict(bound=[-1.0, 1.0]), dict(bound=np.ones(9)),
                dict(cu=np.zeros((2, 4, 3))), dict(off=None)):
        with pytest.raises(ValueError):
            scoring.affine_rows(2, 4, **dict(dict(cx_left=z, cx_right=z, cu=z, off=z, bound=[1.0, 1.0]), **bad))

    class Boom:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name})")

    class Handle:
        ptr, dof = None, 3

    eng = E.Engine.__new__(E.Engine)
    eng.lib = Boom()
    r, y, good = Handle(), Handle(), E.MotionLimits(3, vel=2.0, acc=[1, INF, 3], point_speed=1.5)
    ok = np.zeros((2, 5, 6))
    for bad in (np.zeros((2, 5, 5)), np.zeros((2, 5)), np.zeros((2, 1, 6))):
        with pytest.raises(ValueError):
            eng.retime_dynamic_traj(r, y, good, 0.1, 2, bad)
    for kw in (dict(inter_step=-1), dict(delta_t=0.0), dict(max_rate=0.0), dict(rate_end=NAN), dict(limits=E.MotionLimits(7)),
               dict(out={"sdot": np.zeros((2, 4))}), dict(out={"achieved": np.zeros((2, 4))}),
               dict(out={"coef": np.zeros((2, 9, 3, 4))}), dict(out={"tau": np.zeros((2, 9, 3))})):
        args = dict(dict(limits=good, delta_t=0.1, inter_step=1), **kw)
        with pytest.raises(ValueError):
            eng.retime_dynamic_traj(r, y, traj=ok, **args)
    q, cap, rows = np.zeros((2, 4, 3)), np.ones((2, 4)), np.zeros((2, 4, 2))
    for kw in (dict(qd=np.zeros((2, 1, 3))), dict(cap=np.ones((2, 5))), dict(acc=[1.0, 0.0, 1.0]), dict(h=0.0),
               dict(max_rate=NAN), dict(bound=[1.0, -1.0]), dict(bound=np.ones(9)), dict(cu=np.zeros((2, 4, 3))),
               dict(out={"achieved": np.zeros((2, 4))}), dict(out={"dense_retimed": np.zeros((2, 4, 6))})):
        args = dict(dict(qd=q, qdd_left=q, qdd_right=q, cap=cap, acc=None, cx_left=rows, cx_right=rows, cu=rows, off=rows,
                         bound=[1.0, 2.0], h=0.1), **kw)
        with pytest.raises(ValueError):
            eng.retime_path_affine(**args)
    pl = E.Plan.__new__(E.Plan)
    pl.eng, pl.B, pl.N, pl.D = eng, 2, 4, 3
    for call in (pl.retime_dynamic, pl.retime_dynamic_dev):
        with pytest.raises(ValueError):
            call(y, good, -1)
        with pytest.raises(ValueError):
            call(y, good, 1, max_rate=INF)
        with pytest.raises(ValueError):
            call(y, E.MotionLimits(7), 1)
    with pytest.raises(ValueError):
        pl.retime_dynamic(y, good, 1, out={"coef": np.zeros((2, 9, 3))})
    for call in (pl.select_retimed_dynamic, pl.select_retimed_dynamic_dev):
        for kw in (dict(required_pos_margin=NAN), dict(max_duration=NAN), dict(max_rate=0.0), dict(rate_start=-1.0)):
            with pytest.raises(ValueError):
                call(1, good, y, **kw)
        with pytest.raises(ValueError):
            call(-2, good, y)


def test_retimed_dynamic_rule_on_hand_cases():
    fe = np.array([3.0, 1.0, 1.0, 0.5, np.nan])
    st = np.array([0, 0, 0, 3, 0])
    clr, oor = np.full(5, 0.1), np.zeros(5, dtype=np.int32)
    rs, dur = np.zeros(5, dtype=np.int32), np.array([2.0, 3.0, 2.5, 1.0, 1.0])
    rule = scoring.retimed_dynamic_rule
    assert rule(fe, st, clr, oor, retime_status=rs, duration=dur) == scoring.retimed_rule(
        fe, st, clr, oor, retime_status=rs, duration=dur) == (1, 3)
    fin = np.array([True, False, True, True, True])
    assert rule(fe, st, clr, oor, retime_status=rs, duration=dur, coef_finite=fin) == (2, 2)
    assert rule(fe, st, clr, oor, retime_status=np.array([0, 4, 4, 0, 0]), duration=dur) == (0, 1)      # STATIC rows
    assert rule(fe, st, clr, oor, retime_status=rs, duration=dur, max_duration=2.0, coef_finite=~fin) == (-1, 0)


def test_without_a_gpu_the_compute_calls_answer_no_device(eng):
    """gpmp2mi_retime_path_affine starts from no handle: it is the one call of this section that can be made without a
    device, and it answers GPMP2MI_ERR_NO_DEVICE rather than computing elsewhere; the others start from a robot handle,
    and the way to that raises the same"""
    if eng.device_count() > 0:
        return          # only observable without a GPU; with one, tests/test_gpu_retime_dynamic.py runs the calls
    q, cap, rows = np.zeros((1, 3, 2)), np.full((1, 3), INF), np.zeros((1, 3, 1))
    with pytest.raises(E.Gpmp2miError) as ei:
        eng.retime_path_affine(q, q, q, cap, None, rows, rows, rows, rows, [1.0], 0.1)
    assert ei.value.code == 2
    import gpmp2_amd
    from gpmp2_amd import dynamics as tables
    t = tables.illustrative_wam()
    with pytest.raises(E.Gpmp2miError) as ei:
        r = eng.robot(gpmp2_amd.generateArm("WAMArm"))
        y = eng.dynamics(r, t["mass"], t["com"], t["inertia"], torque=t["torque"])
        eng.retime_dynamic_traj(r, y, E.MotionLimits(7, vel=2.0), 0.1, 1, np.zeros((1, 3, 14)))
    assert ei.value.code == 2
