"""Scene (include/gpmp2mi.h "scene") as far as it can be checked without a GPU: the ABI is declared, exported and bound,
every refusal that needs no live handle comes back before any device work with a message that names the trouble and
with the outputs untouched, and the Python objects refuse wrong input before the library is called.  What needs a live
handle -- use_base without a base, use_evidence without evidence, first / count outside the scene -- is in
tests/test_gpu_scene.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scene_cases as sc
from gpmp2_amd import _capi
from gpmp2_amd import engine as E
from gpmp2_amd import scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_NAMES = ["gpmp2mi_scene_create", "gpmp2mi_scene_count", "gpmp2mi_scene_set_poses", "gpmp2mi_scene_set_enabled",
             "gpmp2mi_scene_reserve", "gpmp2mi_scene_rasterize", "gpmp2mi_scene_rasterize_dev",
             "gpmp2mi_sdf_update_from_scene", "gpmp2mi_sdf_update_from_scene_dev"]


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def test_entry_points_and_constants_are_declared_exported_and_bound(eng):
    hdr = open(os.path.join(ROOT, "include", "gpmp2mi.h")).read()
    assert hdr.index("---- sensor map") < hdr.index("---- scene:")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in INT_NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", code), f"{n} is not declared in include/gpmp2mi.h"
        assert hasattr(eng.lib, n), f"{n} is not exported"
        assert getattr(eng.lib, n).argtypes is not None, f"{n} is not bound in _capi.py"
    assert re.search(r"\bvoid\s+gpmp2mi_scene_destroy\s*\(", code) and hasattr(eng.lib, "gpmp2mi_scene_destroy")
    assert re.search(r"typedef\s+struct\s+gpmp2mi_scene_object\s*\{", code)
    m = re.search(r"enum\s*\{\s*GPMP2MI_SCENE_BOX = (\d+), GPMP2MI_SCENE_SPHERE = (\d+), GPMP2MI_SCENE_CYLINDER = (\d+), "
                  r"GPMP2MI_SCENE_MESH = (\d+)\s*\}", code)
    assert m and [int(x) for x in m.groups()] == [_capi.SCENE_BOX, _capi.SCENE_SPHERE, _capi.SCENE_CYLINDER, _capi.SCENE_MESH]
    assert [int(x) for x in m.groups()] == [0, 1, 2, 3]
    assert int(re.search(r"#define GPMP2MI_MAX_SCENE_OBJECTS (\d+)", code).group(1)) == _capi.MAX_SCENE_OBJECTS == 256
    # the struct as the header lays it out: int, double[3], double, int, ptr, int, ptr, double[12], int
    f = {n: getattr(_capi.SceneObject, n).offset for n, _ in _capi.SceneObject._fields_}
    assert [f[k] for k in ("kind", "size", "inflate", "n_vertices", "vertices", "n_triangles", "triangles", "pose",
                           "enabled")] == [0, 8, 32, 40, 48, 56, 64, 72, 168] and C.sizeof(_capi.SceneObject) == 176
    # the rules are written into the header
    for word in ("crossing parity", "ties to even", "sqrt(3) / 2", "Parity is per mesh", "2^29", "(d.y == 0"):
        assert word in hdr, word
    eng.lib.gpmp2mi_scene_destroy(None)                    # a null handle is left alone
    assert eng.lib.gpmp2mi_scene_count(None) == -1


def _raw(obj):
    """a SceneObject struct of a test-case dict without the Python-side checks; keeps its arrays alive"""
    o = _capi.SceneObject()
    o.kind, o.inflate, o.enabled = int(obj["kind"]), float(obj.get("inflate", 0.0)), 1
    for k in range(3):
        o.size[k] = float(obj["size"][k])
    for k, x in enumerate(np.asarray(obj["pose"], dtype=np.float64).reshape(12)):
        o.pose[k] = float(x)
    keep = []
    if obj.get("vertices") is not None:
        v = np.ascontiguousarray(obj["vertices"], dtype=np.float64)
        t = np.ascontiguousarray(obj["triangles"], dtype=np.int32)
        o.n_vertices, o.n_triangles = obj.get("V", len(v)), obj.get("T", len(t))
        o.vertices, o.triangles = v.ctypes.data_as(_capi.c_double_p), t.ctypes.data_as(_capi.c_int_p)
        keep = [v, t]
    return o, keep


def test_create_refuses_bad_objects_before_any_device_work(eng):
    lib = eng.lib
    nan, inf = float("nan"), float("inf")
    good_box = sc.box([0.1, 0.2, 0.3], sc.pose())
    cube = sc.mesh(sc.cube((0, 0, 0), (1, 1, 1)))
    v, t = cube["vertices"], cube["triangles"]

    def with_pose(i, x):
        P = sc.pose()
        P.reshape(12)[i] = x
        return P

    bad = {                                                # name -> (object dict, code, a word of the message)
        "unknown kind": (dict(good_box, kind=4), 1, "kind"),
        "negative kind": (dict(good_box, kind=-1), 1, "kind"),
        "nan pose": (dict(good_box, pose=with_pose(3, nan)), 1, "pose"),
        "inf pose": (dict(good_box, pose=with_pose(0, inf)), 1, "pose"),
        "nan size": (dict(good_box, size=[0.1, nan, 0.3]), 1, "size"),
        "inf size": (sc.sphere(inf, (0, 0, 0)), 1, "size"),
        "negative size": (sc.cylinder(0.1, -0.2, sc.pose()), 1, "size"),
        "nan inflate": (dict(good_box, inflate=nan), 1, "inflate"),
        "negative inflate": (dict(good_box, inflate=-0.01), 1, "inflate"),
        "mesh inflate": (dict(cube, inflate=0.01), 1, "inflate"),
        "mesh V < 4": (dict(cube, V=3), 1, "at least 4"),
        "mesh T < 4": (dict(cube, T=3), 1, "at least 4"),
        "mesh index high": (dict(cube, triangles=np.where(t == 7, 8, t)), 1, "index"),
        "mesh index negative": (dict(cube, triangles=np.where(t == 0, -1, t)), 1, "index"),
        "mesh repeated index": (dict(cube, triangles=np.vstack([t[:-1], [[t[-1][0], t[-1][1], t[-1][1]]]])), 1, "repeated"),
        "mesh open": (dict(cube, triangles=t[:-1]), 1, "not closed"),
        "mesh too many triangles": (dict(cube, T=(1 << 20) + 1), 4, "2^20"),
    }
    sentinel = C.c_void_p(12345)
    for name, (obj, code, word) in bad.items():
        o, keep = _raw(obj)
        out = C.c_void_p(sentinel.value)
        arr = (_capi.SceneObject * 2)(_raw(good_box)[0], o)   # the bad one is not the first
        assert lib.gpmp2mi_scene_create(2, arr, C.byref(out)) == code, name
        assert word in lib.gpmp2mi_last_error().decode(), (name, lib.gpmp2mi_last_error().decode())
        assert out.value == sentinel.value, name              # a refused call writes nothing
    o, _ = _raw(good_box)
    out = C.c_void_p(sentinel.value)
    for K in (0, -1, 257):
        arr = (_capi.SceneObject * 1)(o)
        assert lib.gpmp2mi_scene_create(K, arr, C.byref(out)) == 1 and "K" in lib.gpmp2mi_last_error().decode()
    assert lib.gpmp2mi_scene_create(1, None, C.byref(out)) == 1 and "null" in lib.gpmp2mi_last_error().decode()
    assert lib.gpmp2mi_scene_create(1, (_capi.SceneObject * 1)(o), None) == 1
    null_mesh, _ = _raw(cube)
    null_mesh.vertices = None
    assert lib.gpmp2mi_scene_create(1, (_capi.SceneObject * 1)(null_mesh), C.byref(out)) == 1
    assert out.value == sentinel.value
    # sizes a kind does not use are not read: a sphere with rubbish behind its radius is accepted as far as the checks
    # go -- without a GPU the next complaint is the missing device, with one the scene is made
    sph, _ = _raw(dict(sc.sphere(0.1, (0, 0, 0)), size=[0.1, nan, -1.0]))
    out = C.c_void_p()
    rc = lib.gpmp2mi_scene_create(1, (_capi.SceneObject * 1)(sph), C.byref(out))
    assert rc == (0 if eng.device_count() else 2), lib.gpmp2mi_last_error().decode()
    if rc == 0:
        lib.gpmp2mi_scene_destroy(out)


def test_calls_refuse_bad_arguments_before_a_handle_is_looked_at(eng):
    lib = eng.lib
    one = C.c_void_p(1)          # a non-null handle that must never be looked at: the bad argument is reported first
    nan, inf = float("nan"), float("inf")
    mask = np.full((3, 4, 5), 7, dtype=np.uint8)
    cells = np.full(4, 7, dtype=np.int32)
    m_, c_ = mask.ctypes.data_as(C.POINTER(C.c_ubyte)), E.iptr(cells)

    def rast(s=one, dim=3, origin=(0.0, 0.0, 0.0), cell=0.1, n=(5, 4, 3), m=m_, dev=False):
        o = None if origin is None else E.dptr(np.array(origin, dtype=np.float64))
        if dev:
            return lib.gpmp2mi_scene_rasterize_dev(s, dim, o, cell, *n, one if m is not None else None, None, None)
        return lib.gpmp2mi_scene_rasterize(s, dim, o, cell, *n, m, c_)

    calls = {}
    for dev in (False, True):
        t = " dev" if dev else ""
        calls.update({
            "rasterize scene" + t: (lambda d=dev: rast(s=None, dev=d), "scene"),
            "rasterize mask" + t: (lambda d=dev: rast(m=None, dev=d), "mask"),
            "rasterize origin" + t: (lambda d=dev: rast(origin=None, dev=d), "origin"),
            "rasterize dim" + t: (lambda d=dev: rast(dim=4, dev=d), "dim"),
            "rasterize nx" + t: (lambda d=dev: rast(n=(0, 4, 3), dev=d), "sizes"),
            "rasterize nz" + t: (lambda d=dev: rast(n=(5, 4, -1), dev=d), "sizes"),
            "rasterize planar nz" + t: (lambda d=dev: rast(dim=2, n=(5, 4, 3), dev=d), "planar"),
            "rasterize cell 0" + t: (lambda d=dev: rast(cell=0.0, dev=d), "cell_size"),
            "rasterize cell nan" + t: (lambda d=dev: rast(cell=nan, dev=d), "cell_size"),
            "rasterize cell inf" + t: (lambda d=dev: rast(cell=inf, dev=d), "cell_size"),
            "rasterize origin nan" + t: (lambda d=dev: rast(origin=(0.0, nan, 0.0), dev=d), "origin"),
        })
    upd, upd_dev = lib.gpmp2mi_sdf_update_from_scene, lib.gpmp2mi_sdf_update_from_scene_dev
    calls.update({
        "update field": (lambda: upd(None, one, 0, 0, 1, c_), "field"),
        "update scene": (lambda: upd(one, None, 0, 0, 1, c_), "scene"),
        "update occupied_at": (lambda: upd(one, one, 0, 0, 32768, c_), "occupied_at"),
        "update occupied_at <": (lambda: upd(one, one, 0, 1, -32769, c_), "occupied_at"),
        "update_dev field": (lambda: upd_dev(None, one, 0, 0, 1, None, None), "field"),
        "update_dev scene": (lambda: upd_dev(one, None, 0, 0, 1, None, None), "scene"),
        "update_dev occupied_at": (lambda: upd_dev(one, one, 0, 0, 40000, None, None), "occupied_at"),
        "set_poses scene": (lambda: lib.gpmp2mi_scene_set_poses(None, 0, 1, E.dptr(np.zeros(12))), "scene"),
        "set_enabled scene": (lambda: lib.gpmp2mi_scene_set_enabled(None, 0, 1, E.iptr(np.zeros(1, dtype=np.int32))), "scene"),
        "reserve scene": (lambda: lib.gpmp2mi_scene_reserve(None, 4, 4, 4), "scene"),
        "reserve sizes": (lambda: lib.gpmp2mi_scene_reserve(one, 4, 0, 4), "sizes"),
    })
    for name, (call, word) in calls.items():
        assert call() == 1, name
        msg = lib.gpmp2mi_last_error().decode()
        assert word in msg, (name, msg)
    assert (mask == 7).all() and (cells == 7).all()        # a refused call writes nothing


def test_python_objects_refuse_bad_input_before_the_library_is_called():
    v, t = sc.cube((0, 0, 0), (1, 1, 1))
    for make in (lambda: S.Box([0.1, 0.2]), lambda: S.Box([0.1, -0.2, 0.3]), lambda: S.Sphere(float("nan")),
                 lambda: S.Sphere(0.1, inflate=-1.0), lambda: S.Cylinder(0.1, 0.2, pose=np.zeros((3, 3))),
                 lambda: S.Cylinder(0.1, 0.2, pose=np.full((3, 4), np.inf)), lambda: S.Mesh(v[:3], t),
                 lambda: S.Mesh(v, t[:3]), lambda: S.Mesh(v, t.astype(np.float64)), lambda: S.Mesh(v.reshape(-1), t),
                 lambda: S.Mesh(v, np.where(t == 7, 8, t)), lambda: S.SceneObject(9, [0.1], None),
                 lambda: S.SceneObject(_capi.SCENE_MESH, [], None, 0.01, True, v, t)):
        with pytest.raises(ValueError):
            make()

    class Boom:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name})")

    eng = E.Engine.__new__(E.Engine)
    eng.lib = Boom()
    with pytest.raises(ValueError):
        S.Scene([], eng)
    with pytest.raises(ValueError):
        S.Scene([S.Sphere(0.1)] * 257, eng)
    b = S.Box([0.1, 0.2, 0.3], np.eye(4))                  # a 4 x 4 pose gives its upper rows
    assert b.pose.shape == (3, 4) and b.to_c().size[2] == 0.3 and b.to_c().enabled == 1
    m = S.Mesh(v, t.astype(np.int64), enabled=False).to_c()
    assert (m.n_vertices, m.n_triangles, m.enabled, m.kind) == (8, 12, 0, 3)
