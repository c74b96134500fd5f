"""Planning scene (include/gpmp2mi.h "scene"): boxes, spheres, cylinders and closed triangle meshes with poses, rasterised
on the device into the obstacle set of a field handle.

    table = Box([0.6, 0.4, 0.02], pose_of(t=[0.3, 0.0, -0.02]))
    post = Cylinder(0.04, 0.5, pose_of(t=[0.4, 0.3, 0.5]))
    scene = Scene([table, post, Mesh(vertices, triangles, pose)])
    field.update_from_scene(scene)                # planner.SignedDistanceField / PlanarSDF, or Engine.sdf_update_from_scene
    scene.set_poses([new_pose], first=2)          # the mesh moved
    field.update_from_scene(scene)

Objects are validated here as the C side validates them (ValueError), except the closedness of a mesh, which the library
checks when the scene is made.  Only cell centres are tested: give a thin object an inflate of cell * sqrt(3) / 2 to be
sure that every cell it touches is marked.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi

KIND_NAMES = {_capi.SCENE_BOX: "box", _capi.SCENE_SPHERE: "sphere", _capi.SCENE_CYLINDER: "cylinder",
              _capi.SCENE_MESH: "mesh"}


def pose_of(R=None, t=(0.0, 0.0, 0.0)):
    """[3][4] object -> world from a rotation matrix (None: identity) and a translation"""
    P = np.zeros((3, 4))
    P[:, :3] = np.eye(3) if R is None else np.asarray(R, dtype=np.float64).reshape(3, 3)
    P[:, 3] = np.asarray(t, dtype=np.float64).reshape(3)
    return P


def as_pose(pose):
    """None (identity), [3][4], [4][4] (its upper rows) or 12 numbers -> contiguous float64 [3][4]"""
    if pose is None:
        return pose_of()
    P = np.asarray(pose, dtype=np.float64)
    if P.shape == (4, 4):
        P = P[:3]
    if P.size != 12:
        raise ValueError(f"pose: expected [3][4] (or [4][4]), got {list(P.shape)}")
    return np.ascontiguousarray(P.reshape(3, 4))


def icosphere_mesh(radius=1.0, subdivisions=2):
    """A closed mesh of a sphere: (vertices [V][3], triangles [T][3]) with T = 20 * 4^subdivisions (20 480 at five)"""
    p = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
         (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    v = [np.asarray(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    for _ in range(int(subdivisions)):
        mid, out = {}, []
        for a, b, c in t:
            m = []
            for i, j in ((a, b), (b, c), (c, a)):
                key = (min(i, j), max(i, j))
                if key not in mid:
                    w = v[i] + v[j]
                    v.append(w / np.linalg.norm(w))
                    mid[key] = len(v) - 1
                m.append(mid[key])
            out += [(a, m[0], m[2]), (b, m[1], m[0]), (c, m[2], m[1]), (m[0], m[1], m[2])]
        t = out
    return float(radius) * np.array(v), np.array(t, dtype=np.int32)


class SceneObject:
    """One object of a scene; made by Box, Sphere, Cylinder or Mesh"""

    def __init__(self, kind, size, pose, inflate=0.0, enabled=True, vertices=None, triangles=None):
        if kind not in KIND_NAMES:
            raise ValueError(f"unknown object kind {kind}")
        self.kind = int(kind)
        self.size = np.zeros(3)
        size = np.asarray(size, dtype=np.float64).reshape(-1)
        self.size[:size.size] = size
        self.inflate, self.enabled, self.pose = float(inflate), bool(enabled), as_pose(pose)
        if not (np.isfinite(self.size).all() and np.isfinite(self.inflate) and np.isfinite(self.pose).all()):
            raise ValueError(f"{KIND_NAMES[kind]}: size, inflate and pose must be finite")
        if (self.size < 0).any() or self.inflate < 0:
            raise ValueError(f"{KIND_NAMES[kind]}: size and inflate must be >= 0")
        self.vertices = self.triangles = None
        if kind == _capi.SCENE_MESH:
            if self.inflate != 0.0:
                raise ValueError("mesh: a mesh cannot be inflated")
            v = np.ascontiguousarray(vertices, dtype=np.float64)
            t = np.asarray(triangles)
            if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] < 4:
                raise ValueError(f"mesh vertices: expected [V][3] with V >= 4, got {list(v.shape)}")
            if t.ndim != 2 or t.shape[1] != 3 or t.shape[0] < 4 or not np.issubdtype(t.dtype, np.integer):
                raise ValueError(f"mesh triangles: expected integers [T][3] with T >= 4, got {t.dtype} {list(t.shape)}")
            if t.shape[0] > _capi.MAX_SCENE_TRIANGLES:
                raise ValueError(f"mesh triangles: at most {_capi.MAX_SCENE_TRIANGLES}, got {t.shape[0]}")
            if t.min() < 0 or t.max() >= v.shape[0]:
                raise ValueError("mesh triangles: a vertex index is outside 0 .. V-1")
            self.vertices, self.triangles = v, np.ascontiguousarray(t, dtype=np.int32)

    def to_c(self):
        o = _capi.SceneObject()
        o.kind, o.inflate, o.enabled = self.kind, self.inflate, int(self.enabled)
        for k in range(3):
            o.size[k] = float(self.size[k])
        for k, x in enumerate(self.pose.reshape(12)):
            o.pose[k] = float(x)
        if self.kind == _capi.SCENE_MESH:
            o.n_vertices, o.n_triangles = self.vertices.shape[0], self.triangles.shape[0]
            o.vertices = self.vertices.ctypes.data_as(_capi.c_double_p)
            o.triangles = self.triangles.ctypes.data_as(_capi.c_int_p)
        return o


def Box(half_extents, pose=None, inflate=0.0, enabled=True):
    h = np.asarray(half_extents, dtype=np.float64).reshape(-1)
    if h.size != 3:
        raise ValueError(f"box: expected three half extents, got {h.size}")
    return SceneObject(_capi.SCENE_BOX, h, pose, inflate, enabled)


def Sphere(radius, center=(0.0, 0.0, 0.0), inflate=0.0, enabled=True):
    return SceneObject(_capi.SCENE_SPHERE, [float(radius)], pose_of(t=center), inflate, enabled)


def Cylinder(radius, half_height, pose=None, inflate=0.0, enabled=True):
    """axis along the object's z"""
    return SceneObject(_capi.SCENE_CYLINDER, [float(radius), float(half_height)], pose, inflate, enabled)


def Mesh(vertices, triangles, pose=None, enabled=True):
    """a closed triangle mesh: vertices [V][3] in the object frame, triangles [T][3] vertex indices; any winding"""
    return SceneObject(_capi.SCENE_MESH, [], pose, 0.0, enabled, vertices, triangles)


def as_object(o):
    """a SceneObject, or a dict(kind, size, inflate, pose, enabled, vertices, triangles)"""
    if isinstance(o, SceneObject):
        return o
    return SceneObject(o["kind"], o.get("size", []), o.get("pose"), o.get("inflate", 0.0), o.get("enabled", True),
                       o.get("vertices"), o.get("triangles"))


class Scene:
    """A scene handle on the current device.  `objects`: SceneObjects (or dicts); engine: an engine.Engine (default: a new
    one).  The handle goes with close() or with the object."""

    def __init__(self, objects, engine=None):
        if engine is None:
            from . import engine as _engine
            engine = _engine.Engine()
        self.engine = engine
        self.objects = [as_object(o) for o in objects]
        K = len(self.objects)
        if not 1 <= K <= _capi.MAX_SCENE_OBJECTS:
            raise ValueError(f"a scene holds 1 .. {_capi.MAX_SCENE_OBJECTS} objects, got {K}")
        arr = (_capi.SceneObject * K)(*[o.to_c() for o in self.objects])
        out = C.c_void_p()
        engine._ck(engine.lib.gpmp2mi_scene_create(K, arr, C.byref(out)))
        self.ptr, self.K = out, K

    def close(self):
        if getattr(self, "ptr", None):
            self.engine.lib.gpmp2mi_scene_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self.K

    def _range(self, first, count):
        first = int(first)
        if first < 0 or first + count > self.K:
            raise ValueError(f"objects {first} .. {first + count - 1} are outside the scene of {self.K}")
        return first

    def set_poses(self, poses, first=0):
        """new poses for objects first .. first + len(poses) - 1 (host data: the next call reads them)"""
        P = [as_pose(p) for p in poses]
        first = self._range(first, len(P))
        if not all(np.isfinite(p).all() for p in P):
            raise ValueError("poses must be finite")
        flat = np.ascontiguousarray(np.stack(P).reshape(-1)) if P else np.zeros(0)
        self.engine._ck(self.engine.lib.gpmp2mi_scene_set_poses(self.ptr, first, len(P),
                                                                flat.ctypes.data_as(_capi.c_double_p)))
        for k, p in enumerate(P):
            self.objects[first + k].pose = p

    def set_pose(self, index, pose):
        self.set_poses([pose], index)

    def set_enabled(self, enabled, first=0):
        flags = np.ascontiguousarray([1 if e else 0 for e in np.atleast_1d(enabled)], dtype=np.int32)
        first = self._range(first, len(flags))
        self.engine._ck(self.engine.lib.gpmp2mi_scene_set_enabled(self.ptr, first, len(flags),
                                                                  flags.ctypes.data_as(_capi.c_int_p)))
        for k, e in enumerate(flags):
            self.objects[first + k].enabled = bool(e)

    def reserve(self, shape):
        """takes the workspace for a grid of shape [nz][ny][nx] or [ny][nx] now"""
        nz, ny, nx = ((1,) + tuple(shape)) if len(shape) == 2 else tuple(shape)
        self.engine._ck(self.engine.lib.gpmp2mi_scene_reserve(self.ptr, int(nx), int(ny), int(nz)))

    def rasterize(self, origin, cell_size, shape):
        """The occupied set of the scene alone on a grid of shape [nz][ny][nx] (origin of three numbers) or [ny][nx]
        (two): -> (mask uint8 of that shape, cells [K] int32: the count of each object alone, -1 = mesh out of range)"""
        shape = tuple(int(x) for x in shape)
        origin = np.asarray(origin, dtype=np.float64).reshape(-1)
        if len(shape) not in (2, 3) or origin.size != len(shape) or min(shape) < 1:
            raise ValueError(f"rasterize: a shape of 2 or 3 sizes >= 1 and an origin of as many numbers, got {shape}, "
                             f"{origin.size}")
        dim = len(shape)
        nz, ny, nx = ((1,) + shape) if dim == 2 else shape
        org = np.ascontiguousarray(list(origin) + [0.0] * (3 - dim))
        mask, cells = np.zeros(shape, dtype=np.uint8), np.zeros(self.K, dtype=np.int32)
        self.engine._ck(self.engine.lib.gpmp2mi_scene_rasterize(
            self.ptr, dim, org.ctypes.data_as(_capi.c_double_p), float(cell_size), nx, ny, nz,
            mask.ctypes.data_as(C.POINTER(C.c_ubyte)), cells.ctypes.data_as(_capi.c_int_p)))
        return mask, cells
