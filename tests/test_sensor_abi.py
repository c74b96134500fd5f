"""Sensor map (include/gpmp2mi.h "sensor map") as far as it can be checked without a GPU: the ABI is declared and exported,
the argument errors that need no live handle are reported with a message that names the argument before the handle is
looked at and before any device work, and the Python wrappers refuse wrong shapes before the library is called.  What
needs a live handle -- use_base without a base, a planar handle to the depth form, a non-finite sensor origin (its length
is the handle's), another device -- is in tests/test_gpu_sensor.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpmp2_amd import _capi
from gpmp2_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_NAMES = ["gpmp2mi_sdf_reserve_evidence", "gpmp2mi_sdf_integrate_points", "gpmp2mi_sdf_integrate_points_dev",
             "gpmp2mi_sdf_integrate_depth", "gpmp2mi_sdf_integrate_depth_dev", "gpmp2mi_sdf_refresh_from_evidence",
             "gpmp2mi_sdf_refresh_from_evidence_dev", "gpmp2mi_sdf_evidence_reset", "gpmp2mi_sdf_evidence_reset_dev",
             "gpmp2mi_sdf_get_evidence"]


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def _opts(**kw):
    return E.Engine._evidence_opts(kw)


def _cam(**kw):
    cam = dict(width=4, height=3, fx=30.0, fy=30.0, cx=1.5, cy=1.0, depth_min=0.1, depth_max=2.0,
               pose=np.eye(4)[:3].copy())
    pose = kw.pop("pose_entry", None)
    cam.update(kw)
    if pose is not None:
        cam["pose"][pose[0], pose[1]] = pose[2]
    return E.Engine._camera(cam)


def test_entry_points_are_declared_and_exported(eng):
    hdr = open(os.path.join(ROOT, "include", "gpmp2mi.h")).read()
    assert "sensor map" in hdr and hdr.index("---- live map") < hdr.index("---- sensor map")
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in INT_NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr), f"{n} is not declared in include/gpmp2mi.h"
        assert hasattr(eng.lib, n), f"{n} is not exported"
    assert re.search(r"\bvoid\s+gpmp2mi_evidence_opts_default\s*\(", hdr) and hasattr(eng.lib, "gpmp2mi_evidence_opts_default")
    for struct in ("gpmp2mi_evidence_opts", "gpmp2mi_depth_camera"):
        assert re.search(r"typedef\s+struct\s+" + struct + r"\s*\{", hdr), struct


def test_default_opts_are_the_headers_and_the_wrappers(eng):
    o = _capi.EvidenceOpts()
    eng.lib.gpmp2mi_evidence_opts_default(C.byref(o))
    got = {k: getattr(o, k) for k, _ in _capi.EvidenceOpts._fields_}
    assert got == dict(hit=2, miss=1, lo=-4, hi=8, occupied_at=1, use_base=0, refresh=1)
    assert got == {k: int(v) for k, v in E.Engine.EVIDENCE_DEFAULTS.items()}
    eng.lib.gpmp2mi_evidence_opts_default(None)            # a null pointer is left alone


def test_bad_arguments_are_refused_before_the_handle_is_looked_at(eng):
    lib = eng.lib
    one = C.c_void_p(1)   # a non-null handle that must never be looked at: the bad argument is reported first
    pts, org, conf, depth = np.zeros((2, 3)), np.zeros(3), np.zeros(7), np.zeros((3, 4), dtype=np.float32)
    stats = np.full(6, 7, dtype=np.int32)
    p_, o_, q_, s_ = E.dptr(pts), E.dptr(org), E.dptr(conf), E.iptr(stats)
    z_ = depth.ctypes.data_as(C.POINTER(C.c_float))
    nan, inf = float("nan"), float("inf")
    ok, cam = C.byref(_opts()), C.byref(_cam())

    def points(s=one, M=2, p=p_, o=o_, robot=None, q=None, margin=0.0, opts=ok, dev=False):
        if dev:
            return lib.gpmp2mi_sdf_integrate_points_dev(s, M, one if p is not None else None, o, robot,
                                                        one if q is not None else None, margin, opts, None, None)
        return lib.gpmp2mi_sdf_integrate_points(s, M, p, o, robot, q, margin, opts, s_)

    def image(s=one, c=cam, z=z_, robot=None, q=None, margin=0.0, opts=ok, dev=False):
        if dev:
            return lib.gpmp2mi_sdf_integrate_depth_dev(s, c, one if z is not None else None, robot,
                                                       one if q is not None else None, margin, opts, None, None)
        return lib.gpmp2mi_sdf_integrate_depth(s, c, z, robot, q, margin, opts, s_)

    bad_opts = {
        "opts.hit": _opts(hit=-1), "opts.miss": _opts(miss=-1), "opts.lo": _opts(lo=1), "opts.lo ": _opts(lo=-32769),
        "opts.hi": _opts(hi=-1), "opts.hi ": _opts(hi=32768), "opts.occupied_at": _opts(occupied_at=-4),
        "opts.occupied_at ": _opts(occupied_at=9),
    }
    bad_cams = {
        "width": _cam(width=-1), "height": _cam(height=-4), "INT_MAX": _cam(width=65536, height=65536),
        "intrinsics": _cam(fx=nan), "intrinsics ": _cam(cy=inf), "fx": _cam(fx=0.0), "fy": _cam(fy=0.0),
        "depth range": _cam(depth_min=-0.1), "depth range ": _cam(depth_min=2.0, depth_max=2.0),
        "depth range  ": _cam(depth_max=inf), "depth range   ": _cam(depth_min=nan), "pose": _cam(pose_entry=(1, 3, nan)),
        "pose ": _cam(pose_entry=(0, 0, inf)),
    }
    calls = {}                                             # name -> (call, a word its message must hold)
    for dev in (False, True):
        t = " dev" if dev else ""
        calls.update({
            "points handle" + t: (lambda d=dev: points(s=None, dev=d), "handle"),
            "points opts" + t: (lambda d=dev: points(opts=None, dev=d), "opts"),
            "points M < 0" + t: (lambda d=dev: points(M=-1, dev=d), "M"),
            "points null" + t: (lambda d=dev: points(p=None, dev=d), "points"),
            "points origin" + t: (lambda d=dev: points(o=None, dev=d), "sensor_origin"),
            "points margin" + t: (lambda d=dev: points(margin=nan, dev=d), "margin"),
            "points conf" + t: (lambda d=dev: points(robot=one, dev=d), "conf"),
            "depth handle" + t: (lambda d=dev: image(s=None, dev=d), "handle"),
            "depth opts" + t: (lambda d=dev: image(opts=None, dev=d), "opts"),
            "depth camera" + t: (lambda d=dev: image(c=None, dev=d), "camera"),
            "depth null" + t: (lambda d=dev: image(z=None, dev=d), "depth"),
            "depth margin" + t: (lambda d=dev: image(margin=nan, dev=d), "margin"),
            "depth conf" + t: (lambda d=dev: image(robot=one, dev=d), "conf"),
        })
        for name, o in bad_opts.items():
            calls[f"points {name}{t}"] = (lambda d=dev, o=o: points(opts=C.byref(o), dev=d), name.strip())
            calls[f"depth {name}{t}"] = (lambda d=dev, o=o: image(opts=C.byref(o), dev=d), name.strip())
        for name, c in bad_cams.items():
            calls[f"camera {name}{t}"] = (lambda d=dev, c=c: image(c=C.byref(c), dev=d), name.strip())
    calls.update({
        "reserve handle": (lambda: lib.gpmp2mi_sdf_reserve_evidence(None), "handle"),
        "refresh handle": (lambda: lib.gpmp2mi_sdf_refresh_from_evidence(None, 1, 0), "handle"),
        "refresh occupied_at": (lambda: lib.gpmp2mi_sdf_refresh_from_evidence(one, 32768, 0), "occupied_at"),
        "refresh occupied_at <": (lambda: lib.gpmp2mi_sdf_refresh_from_evidence(one, -32769, 0), "occupied_at"),
        "refresh_dev handle": (lambda: lib.gpmp2mi_sdf_refresh_from_evidence_dev(None, 1, 0, None), "handle"),
        "refresh_dev occupied_at": (lambda: lib.gpmp2mi_sdf_refresh_from_evidence_dev(one, 40000, 0, None), "occupied_at"),
        "reset handle": (lambda: lib.gpmp2mi_sdf_evidence_reset(None), "handle"),
        "reset_dev handle": (lambda: lib.gpmp2mi_sdf_evidence_reset_dev(None, None), "handle"),
        "get handle": (lambda: lib.gpmp2mi_sdf_get_evidence(None, None), "handle"),
        "get E": (lambda: lib.gpmp2mi_sdf_get_evidence(one, None), "E"),
    })
    assert len(calls) == 2 * (13 + 2 * len(bad_opts) + len(bad_cams)) + 10     # no name was used twice
    for name, (call, word) in calls.items():
        assert call() == 1, name
        msg = lib.gpmp2mi_last_error().decode()
        assert word in msg, (name, msg)
    assert stats.tolist() == [7] * 6                       # a refused call writes nothing
    # the edges of the ranges are accepted as far as the argument checks go: the next complaint is about something else
    edge = _opts(hit=0, miss=0, lo=-32768, hi=32767, occupied_at=-32767)
    assert points(opts=C.byref(edge), p=None) == 1 and "points" in lib.gpmp2mi_last_error().decode()
    edge = _opts(lo=0, hi=0, occupied_at=0)
    assert points(opts=C.byref(edge), p=None) == 1 and "occupied_at" in lib.gpmp2mi_last_error().decode()   # lo < occupied_at


def test_python_wrappers_refuse_bad_input_before_the_library_is_called():
    class Boom:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name})")

    class Field:
        ptr, dim, shape = None, 3, (4, 5, 6)

    class Robot:
        ptr, dof, S = None, 7, 16

    eng = E.Engine.__new__(E.Engine)
    eng.lib = Boom()
    s, r = Field(), Robot()
    good, o = np.zeros((5, 3)), np.zeros(3)
    for bad in (np.zeros((5, 2)), np.zeros(6), np.zeros((2, 3, 3))):
        with pytest.raises(ValueError):
            eng.sdf_integrate_points(s, bad, o)
    for bad_o in (np.zeros(2), np.zeros(4), np.zeros((2, 3))):
        with pytest.raises(ValueError):
            eng.sdf_integrate_points(s, good, bad_o)
        with pytest.raises(ValueError):
            eng.sdf_integrate_points_dev(s, 5, 1, bad_o)
    with pytest.raises(ValueError):
        eng.sdf_integrate_points(s, good, o, robot=r)                          # a robot without its configuration
    with pytest.raises(ValueError):
        eng.sdf_integrate_points(s, good, o, robot=r, conf=np.zeros(6))
    with pytest.raises(ValueError):
        eng.sdf_integrate_points(s, good, o, margin=float("nan"))
    with pytest.raises(ValueError):
        eng.sdf_integrate_points(s, good, o, hits=3)                           # an unknown option
    with pytest.raises(ValueError):
        eng.sdf_integrate_points_dev(s, -1, 1, o)
    with pytest.raises(ValueError):
        eng.sdf_integrate_points_dev(s, 5, 1, o, robot=r)
    cam = dict(width=4, height=3, fx=30.0, fy=30.0, cx=1.5, cy=1.0, depth_min=0.1, depth_max=2.0, pose=np.eye(4)[:3])
    for bad in (np.zeros((4, 3)), np.zeros(12), np.zeros((3, 4, 1))):
        with pytest.raises(ValueError):
            eng.sdf_integrate_depth(s, cam, bad)
    with pytest.raises(ValueError):
        eng.sdf_integrate_depth(s, dict(cam, pose=np.eye(4)), np.zeros((3, 4)))
    with pytest.raises(ValueError):
        eng.sdf_integrate_depth(s, cam, np.zeros((3, 4)), robot=r)
    with pytest.raises(ValueError):
        eng.sdf_integrate_depth(s, cam, np.zeros((3, 4)), margin=float("nan"))
    with pytest.raises(ValueError):
        eng.sdf_integrate_depth_dev(s, cam, 1, robot=r)
    planar = Field()
    planar.dim, planar.shape = 2, (5, 6)
    with pytest.raises(ValueError):
        eng.sdf_integrate_points(planar, good, np.zeros(2))
    with pytest.raises(ValueError):
        eng.sdf_integrate_depth(planar, cam, np.zeros((3, 4)))
