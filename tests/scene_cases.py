"""Shared inputs of the scene tests (include/gpmp2mi.h "scene"): the grids, closed meshes built here (cube, tetrahedron,
icosphere, torus), poses and the object dicts that tests/scene_reference.py and gpmp2_amd.scene both take."""
import numpy as np

import scene_reference as sr

# the grid of the known answers: nx one past a word
GRID_MAIN, ORIGIN_MAIN, CELL_MAIN = (33, 20, 16), (-0.5, -0.3, -0.2), 0.05
# (n, origin, cell): two words exactly / a long row in few columns / three words and a single layer as a 3-D grid / planar
GRIDS = {
    "33x20x16": (GRID_MAIN, ORIGIN_MAIN, CELL_MAIN),
    "64x5x3": ((64, 5, 3), (-0.8, -0.1, -0.05), 0.025),
    "70x9x1": ((70, 9, 1), (-0.7, -0.2, 0.0), 0.02),
    "40x30": ((40, 30), (-0.5, -0.4), 0.025),
}


def pose(R=None, t=(0.0, 0.0, 0.0)):
    P = np.zeros((3, 4))
    P[:, :3] = np.eye(3) if R is None else R
    P[:, 3] = t
    return P


def rotation(axis, angle):
    """Rodrigues: a general rotation about `axis` by `angle`"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


R_GENERAL = rotation((0.3, -0.5, 0.8), 0.7)


def cube(lo, hi):
    """12 triangles, outward winding"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    v = np.array([[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)])
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    t = []
    for a, b, c, d in quads:
        t += [(a, b, c), (a, c, d)]
    return v, np.array(t, dtype=np.int32)


def lattice_cube(n=GRID_MAIN, origin=ORIGIN_MAIN, cell=CELL_MAIN, lo=(4, 3, 2), hi=(10, 9, 8)):
    """a cube whose corners sit on cell centres"""
    o = np.asarray(origin, dtype=np.float64)
    return cube(o + np.asarray(lo) * cell, o + np.asarray(hi) * cell)


def tetrahedron(scale=0.2):
    v = scale * np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
    return v, np.array([(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)], dtype=np.int32)


def icosphere(radius=0.17, subdivisions=2):
    """20 * 4^subdivisions triangles: 320 at two subdivisions"""
    p = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
         (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    v = [np.asarray(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    for _ in range(subdivisions):
        mid, out = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in t:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = out
    return radius * np.array(v), np.array(t, dtype=np.int32)


TORUS_R, TORUS_r = 0.25, 0.1


def torus(R=TORUS_R, r=TORUS_r, nu=24, nv=12):
    """nu x nv quads, two triangles each; axis z, vertices on the analytic torus"""
    u = 2 * np.pi * np.arange(nu) / nu
    w = 2 * np.pi * np.arange(nv) / nv
    v = np.array([[(R + r * np.cos(b)) * np.cos(a), (R + r * np.cos(b)) * np.sin(a), r * np.sin(b)] for a in u for b in w])
    t = []
    for i in range(nu):
        for j in range(nv):
            a, b = i * nv + j, i * nv + (j + 1) % nv
            c, d = ((i + 1) % nu) * nv + (j + 1) % nv, ((i + 1) % nu) * nv + j
            t += [(a, d, c), (a, c, b)]
    return v, np.array(t, dtype=np.int32)


def torus_distance(points, P, R=TORUS_R, r=TORUS_r):
    """signed distance of world points to the analytic torus under pose P (negative inside)"""
    P = np.asarray(P, dtype=np.float64).reshape(3, 4)
    l = (np.asarray(points, dtype=np.float64) - P[:, 3]) @ P[:, :3]
    return np.hypot(np.hypot(l[..., 0], l[..., 1]) - R, l[..., 2]) - r


def shuffled(triangles, seed=3):
    """the same surface: triangles in another order, vertices rotated or swapped within each (any winding)"""
    rng = np.random.default_rng(seed)
    t = np.asarray(triangles)[rng.permutation(len(triangles))].copy()
    for row in t:
        row[:] = row[rng.permutation(3)]
    return np.ascontiguousarray(t, dtype=np.int32)


def box(half, P, inflate=0.0, enabled=True):
    return dict(kind=sr.BOX, size=list(half), inflate=inflate, pose=np.asarray(P, dtype=np.float64), enabled=enabled)


def sphere(radius, t, inflate=0.0, enabled=True):
    return dict(kind=sr.SPHERE, size=[radius, 0.0, 0.0], inflate=inflate, pose=pose(t=t), enabled=enabled)


def cylinder(radius, half_height, P, inflate=0.0, enabled=True):
    return dict(kind=sr.CYLINDER, size=[radius, half_height, 0.0], inflate=inflate, pose=np.asarray(P, dtype=np.float64),
                enabled=enabled)


def mesh(vt, P=None, enabled=True):
    v, t = vt
    return dict(kind=sr.MESH, size=[0.0, 0.0, 0.0], inflate=0.0, pose=pose() if P is None else np.asarray(P, dtype=np.float64),
                vertices=np.ascontiguousarray(v, dtype=np.float64), triangles=np.ascontiguousarray(t, dtype=np.int32),
                enabled=enabled)


def centre_of(n, origin, cell):
    """the middle of the grid in the world (z = 0 on a planar grid)"""
    n3, o = sr.grid3(n), sr.origin3(n, origin)
    c = o + 0.5 * (np.asarray(n3) - 1) * cell
    if len(n) == 2:
        c[2] = 0.0
    return c


TORUS_POSE_MAIN = pose(rotation((1.0, 0.4, 0.2), 0.9), (-0.4, 0.18, 0.18))     # cut by the -x face of the main grid
