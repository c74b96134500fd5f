"""Numpy / Python-integer restatement of the rules of include/gpmp2mi.h "scene": cell centres, the three primitives, and
the solid fill of a closed mesh by crossing parity along x in exact integers.  TEST INFRASTRUCTURE ONLY; written from
the header's text, expression by expression, in IEEE double and int64 (every integer of the rule has at most 62 bits).
A crossing here flips the tail of its row, literally as the rule says; nothing of the kernels' bit volume is mirrored."""
import numpy as np

BOX, SPHERE, CYLINDER, MESH = 0, 1, 2, 3
FIXED_MAX = 2.0 ** 29


def grid3(n):
    """(nx, ny) or (nx, ny, nz) -> (nx, ny, nz); a planar grid has nz = 1"""
    n = tuple(int(x) for x in n)
    return n if len(n) == 3 else n + (1,)


def origin3(n, origin):
    """origin_z counts as 0 on a planar grid"""
    o = [float(x) for x in origin]
    return np.array(o[:2] + [o[2] if len(n) == 3 else 0.0], dtype=np.float64)


def cell_centres(n, origin, cell):
    """-> cx [nx], cy [ny], cz [nz]: origin + index * cell; c_z = 0 on a planar grid"""
    nx, ny, nz = grid3(n)
    o, cell = origin3(n, origin), np.float64(cell)
    cx = o[0] + np.arange(nx, dtype=np.float64) * cell
    cy = o[1] + np.arange(ny, dtype=np.float64) * cell
    cz = o[2] + np.arange(nz, dtype=np.float64) * cell if len(n) == 3 else np.zeros(1)
    return cx, cy, cz


def primitive_mask(kind, size, inflate, pose, n, origin, cell):
    """bool [nz][ny][nx] of one primitive"""
    P = np.asarray(pose, dtype=np.float64).reshape(3, 4)
    R, t = P[:, :3], P[:, 3]
    cx, cy, cz = cell_centres(n, origin, cell)
    d0 = (cx - t[0])[None, None, :]
    d1 = (cy - t[1])[None, :, None]
    d2 = (cz - t[2])[:, None, None]
    s = [np.float64(size[k]) + np.float64(inflate) for k in range(3)]
    with np.errstate(over="ignore", invalid="ignore"):
        if kind == SPHERE:
            return np.sqrt((d0 * d0 + d1 * d1) + d2 * d2) <= s[0]
        l = [(R[0, m] * d0 + R[1, m] * d1) + R[2, m] * d2 for m in range(3)]
        if kind == BOX:
            return (np.abs(l[0]) <= s[0]) & (np.abs(l[1]) <= s[1]) & (np.abs(l[2]) <= s[2])
        assert kind == CYLINDER
        return (np.sqrt(l[0] * l[0] + l[1] * l[1]) <= s[0]) & (np.abs(l[2]) <= s[1])


def quantize(vertices, pose, n, origin, cell):
    """-> q int64 [V][3], or None when the whole-mesh guard fires"""
    P = np.asarray(pose, dtype=np.float64).reshape(3, 4)
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    o = origin3(n, origin)
    with np.errstate(over="ignore", invalid="ignore"):
        w = np.stack([((P[m, 0] * v[:, 0] + P[m, 1] * v[:, 1]) + P[m, 2] * v[:, 2]) + P[m, 3] for m in range(3)], axis=1)
        g = (w - o[None, :]) / np.float64(cell)
        s = g * 1024.0
        if not np.isfinite(g).all() or (np.abs(s) > FIXED_MAX).any():
            return None
    return np.rint(s).astype(np.int64)           # ties to even


def orient(P0, P1, P2):
    """step 5: -> (P0, P1, P2, a) with a > 0, or None for a == 0; Python integers"""
    P0, P1, P2 = ([int(x) for x in P] for P in (P0, P1, P2))
    a = (P1[1] - P0[1]) * (P2[2] - P0[2]) - (P1[2] - P0[2]) * (P2[1] - P0[1])
    if a == 0:
        return None
    if a < 0:
        P1, P2, a = P2, P1, -a
    return P0, P1, P2, a


def edge_passes(e, dy, dz):
    return e > 0 or (e == 0 and (dy > 0 or (dy == 0 and dz > 0)))


def column(P0, P1, P2, a, Y, Z):
    """steps 6 and 7 for one column in Python integers: -> None (no crossing) or first = ceil(x) as a float"""
    e = []
    for A, B in ((P1, P2), (P2, P0), (P0, P1)):
        dy, dz = B[1] - A[1], B[2] - A[2]
        ek = dy * (Z - A[2]) - dz * (Y - A[1])
        if not edge_passes(ek, dy, dz):
            return None
        e.append(ek)
    assert e[0] + e[1] + e[2] == a
    X = [np.float64(P[0]) / np.float64(1024.0) for P in (P0, P1, P2)]
    x = ((np.float64(e[0]) * X[0] + np.float64(e[1]) * X[1]) + np.float64(e[2]) * X[2]) / np.float64(a)
    return float(np.ceil(x))


def _floor_cell(v):
    return v // 1024


def _ceil_cell(v):
    return -((-v) // 1024)


def mesh_mask(vertices, triangles, pose, n, origin, cell):
    """bool [nz][ny][nx] of one closed mesh, or None when it is out of range"""
    nx, ny, nz = grid3(n)
    q = quantize(vertices, pose, n, origin, cell)
    if q is None:
        return None
    flips = np.zeros((nz, ny, nx), dtype=np.uint8)
    for tri in np.asarray(triangles, dtype=np.int64).reshape(-1, 3):
        o = orient(q[tri[0]], q[tri[1]], q[tri[2]])
        if o is None:
            continue
        P0, P1, P2, a = o
        ys, zs = [P[1] for P in (P0, P1, P2)], [P[2] for P in (P0, P1, P2)]
        # a column outside the projected bounding box fails an edge test: only the others need a look
        for k in range(max(_ceil_cell(min(zs)), 0), min(_floor_cell(max(zs)), nz - 1) + 1):
            for j in range(max(_ceil_cell(min(ys)), 0), min(_floor_cell(max(ys)), ny - 1) + 1):
                first = column(P0, P1, P2, a, 1024 * j, 1024 * k)
                if first is None or first >= nx:
                    continue
                flips[k, j, max(int(first), 0):] ^= 1
    return flips.astype(bool)


def object_mask(obj, n, origin, cell):
    """obj: dict(kind, size, inflate, pose, vertices, triangles, enabled) -> (bool mask, cells)"""
    nx, ny, nz = grid3(n)
    if not obj.get("enabled", True):
        return np.zeros((nz, ny, nx), dtype=bool), 0
    if obj["kind"] == MESH:
        m = mesh_mask(obj["vertices"], obj["triangles"], obj["pose"], n, origin, cell)
        if m is None:
            return np.zeros((nz, ny, nx), dtype=bool), -1
    else:
        m = primitive_mask(obj["kind"], obj["size"], obj.get("inflate", 0.0), obj["pose"], n, origin, cell)
    return m, int(m.sum())


def rasterize(objects, n, origin, cell):
    """-> (mask uint8 [nz][ny][nx] or [ny][nx], cells [K]): the union over the enabled objects, the count of each alone"""
    nx, ny, nz = grid3(n)
    mask = np.zeros((nz, ny, nx), dtype=bool)
    cells = []
    for obj in objects:
        m, c = object_mask(obj, n, origin, cell)
        mask |= m
        cells.append(c)
    mask = mask.astype(np.uint8)
    return (mask if len(n) == 3 else mask[0]), cells


def occupied_set(mask, base=None, E=None, occupied_at=1):
    """indicator (float64 0 / 1) of scene U base U {E >= occupied_at}"""
    occ = np.asarray(mask) > 0
    if base is not None:
        occ = occ | (np.asarray(base) > 0.75)
    if E is not None:
        occ = occ | (np.asarray(E) >= occupied_at)
    return occ.astype(np.float64)
