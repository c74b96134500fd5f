"""Numpy / plain Python restatement of rules 1-7 of include/gpmp2mi.h "sensor map": deprojection, cell coordinates, the
class of a ray in its order, the voxel walk, the apply rule, the occupied set and the stats.  The field of the occupied
set comes from map_reference.field_of (the oracle's distance transform).  TEST INFRASTRUCTURE ONLY; every expression is
written as the header writes it, in IEEE double (Python floats and float64 arrays, one rounding per operation)."""
import math

import numpy as np

import map_reference as mr

HIT, INVALID, MAX_RANGE, SELF, OUTSIDE = 0, 1, 2, 3, 4
STAT_NAMES = ("hit", "invalid", "max_range", "self", "outside", "occupied")
DEFAULTS = dict(hit=2, miss=1, lo=-4, hi=8, occupied_at=1, use_base=False, refresh=True)
MAX_SPAN = 1048576.0


def options(**kw):
    assert set(kw) <= set(DEFAULTS), kw
    return dict(DEFAULTS, **kw)


# ------------------------------------------------------------------------------------------------ rule 1
def deproject(cam, z, u=None, v=None):
    """world points [M][3] of the pixels (u column, v row; all pixels row by row when None) at depths z [M] (float64)"""
    if u is None:
        v, u = np.divmod(np.arange(cam["width"] * cam["height"]), cam["width"])
    P = np.asarray(cam["pose"], dtype=np.float64).reshape(3, 4)
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        xc = ((u.astype(np.float64) - np.float64(cam["cx"])) / np.float64(cam["fx"])) * z
        yc = ((v.astype(np.float64) - np.float64(cam["cy"])) / np.float64(cam["fy"])) * z
        return np.stack([((P[i, 0] * xc + P[i, 1] * yc) + P[i, 2] * z) + P[i, 3] for i in range(3)], axis=1)


def camera_origin(cam):
    return np.asarray(cam["pose"], dtype=np.float64).reshape(3, 4)[:, 3].copy()


# ------------------------------------------------------------------------------------------------ rules 2 and 3
def _span_too_long(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        return ~(np.abs(b - a[None, :]) < MAX_SPAN).all(axis=1)


def classify(n, origin, cell, sensor_origin, points, z=None, cam=None, centers=None, radii=None, margin=0.0):
    """-> (cls [M], a [dim], b [M][dim], end points [M][dim]).  `points` are the given points, or with z / cam the
    deprojected pixels at their own depth; b and the end points of max_range rays are the recomputed ones."""
    dim = len(n)
    p = np.array(points, dtype=np.float64).reshape(-1, dim)
    M = p.shape[0]
    o = np.asarray(sensor_origin, dtype=np.float64).reshape(dim)
    a = mr.cell_coordinate(o[None, :], origin, cell)[0]
    cls = np.full(M, -1, dtype=np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        if z is not None:
            z = np.asarray(z, dtype=np.float64).reshape(-1)
            cls[~np.isfinite(z) | (z <= 0.0) | (z < np.float64(cam["depth_min"]))] = INVALID
        else:
            cls[~np.isfinite(p).all(axis=1)] = INVALID
        b = mr.cell_coordinate(p, origin, cell)
        cls[(cls < 0) & _span_too_long(a, b)] = INVALID
        if z is not None:
            far = (cls < 0) & (z > np.float64(cam["depth_max"]))
            if far.any():
                v, u = np.divmod(np.arange(M), cam["width"])
                p[far] = deproject(cam, np.full(int(far.sum()), np.float64(cam["depth_max"])), u[far], v[far])
                b[far] = mr.cell_coordinate(p[far], origin, cell)
                cls[far] = MAX_RANGE
                cls[far & _span_too_long(a, b)] = INVALID
        if centers is not None and M:
            limit = np.asarray(radii, dtype=np.float64) + np.float64(margin)
            inside_body = (mr.sphere_distance(p, centers) <= limit[None, :]).any(axis=1)
            cls[(cls < 0) & inside_body] = SELF
        in_grid = ((b >= 0.0) & (b < np.asarray(n, dtype=np.float64)[None, :])).all(axis=1)
    cls[(cls < 0) & ~in_grid] = OUTSIDE
    cls[cls < 0] = HIT
    return cls, a, b, p


# ------------------------------------------------------------------------------------------------ rule 4
def walk(a, b):
    """the cells (tuples of ints, x first) of the walk from cell coordinates a to b, the start cell first"""
    dim = len(a)
    a, b = [float(x) for x in a], [float(x) for x in b]
    c = [math.floor(x) for x in a]
    e = [math.floor(x) for x in b]
    left = [abs(e[k] - c[k]) for k in range(dim)]
    step = [(e[k] > c[k]) - (e[k] < c[k]) for k in range(dim)]
    inv, first = [0.0] * dim, [0.0] * dim
    for k in range(dim):
        if left[k] > 0:
            d = b[k] - a[k]
            inv[k] = 1.0 / abs(d)                                   # a float division: inf for a denormal d
            first[k] = (c[k] + 1.0) - a[k] if step[k] > 0 else a[k] - c[k]
    j = [0] * dim
    cells = [tuple(c)]
    for _ in range(sum(left)):
        # the axis with the smallest t among those with steps left, ties to the lowest index: axis k is taken iff
        # t_k <= t_m for every later axis m with steps left and no earlier axis was taken (a comparison with a NaN t is
        # false, so such an axis is taken last)
        active = [k for k in range(dim) if j[k] < left[k]]
        t = [(first[k] + float(j[k])) * inv[k] for k in active]
        best = active[-1]
        for pos in range(len(active) - 1):
            if all(t[pos] <= t[m] for m in range(pos + 1, len(active))):
                best = active[pos]
                break
        c[best] += step[best]
        j[best] += 1
        cells.append(tuple(c))
    assert c == e, (a, b, c, e)
    return cells


# ------------------------------------------------------------------------------------------------ rules 4-5: marks, apply
def marks_of(n, cls, a, b):
    """(miss, hit) bool arrays [nz][ny][nx] / [ny][nx] of one call"""
    shape = mr.grid_shape(n)
    miss, hit = np.zeros(shape, dtype=bool), np.zeros(shape, dtype=bool)
    dim = len(n)

    def inside(c):
        return all(0 <= c[k] < n[k] for k in range(dim))

    for i in range(len(cls)):
        if cls[i] == INVALID:
            continue
        cells = walk(a, b[i])
        for c in cells[:-1]:
            if inside(c):
                miss[c[::-1]] = True
        if cls[i] == HIT:
            assert inside(cells[-1])
            hit[cells[-1][::-1]] = True
    return miss, hit


def marks_of_batch(n, cls, a, b):
    """marks_of with all rays stepping together (numpy over the rays, one walk step per iteration): the same rule, for
    frames too large for the ray-by-ray form.  tests/test_sensor_cpu.py holds the two against each other."""
    dim, nn = len(n), np.asarray(n, dtype=np.int64)
    shape = mr.grid_shape(n)
    miss, hit = np.zeros(shape, dtype=bool), np.zeros(shape, dtype=bool)
    rows = np.flatnonzero(np.asarray(cls) != INVALID)
    if len(rows) == 0:
        return miss, hit
    A, B = np.broadcast_to(np.asarray(a, dtype=np.float64), (len(rows), dim)), np.asarray(b, dtype=np.float64)[rows]
    c, e = np.floor(A).astype(np.int64), np.floor(B).astype(np.int64)
    left, step = np.abs(e - c), np.sign(e - c)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        inv = np.where(left > 0, 1.0 / np.abs(B - A), 0.0)
    first = np.where(step > 0, (c + 1.0) - A, A - c)
    j = np.zeros_like(left)
    act = np.flatnonzero(left.sum(axis=1) > 0)

    def store(vol, cells):
        ok = ((cells >= 0) & (cells < nn[None, :])).all(axis=1)
        vol[tuple(cells[ok][:, k] for k in range(dim - 1, -1, -1))] = True

    while len(act):
        store(miss, c[act])                                        # the cell before the step: never the last cell
        has = j[act] < left[act]
        with np.errstate(invalid="ignore", over="ignore"):
            t = (first[act] + j[act].astype(np.float64)) * inv[act]
            best, taken = np.full(len(act), dim - 1), np.zeros(len(act), dtype=bool)
            for k in range(dim - 1):
                ok = has[:, k] & ~taken
                for m in range(k + 1, dim):
                    ok &= ~has[:, m] | (t[:, k] <= t[:, m])
                best[ok] = k
                taken |= ok
        c[act, best] += step[act, best]
        j[act, best] += 1
        act = act[(j[act] < left[act]).any(axis=1)]
    assert (c == e).all()
    store(hit, e[np.asarray(cls)[rows] == HIT])
    return miss, hit


def apply(E, miss, hit, opts):
    """E' = clamp(E + (hit ? +hit : miss ? -miss : 0), lo, hi) as int16"""
    delta = np.where(hit, int(opts["hit"]), np.where(miss, -int(opts["miss"]), 0))
    return np.clip(E.astype(np.int64) + delta, int(opts["lo"]), int(opts["hi"])).astype(np.int16)


def stats_of(cls, E, opts):
    st = {name: int((cls == k).sum()) for k, name in enumerate(STAT_NAMES[:5])}
    st["occupied"] = int((E >= int(opts["occupied_at"])).sum())
    return st


# ------------------------------------------------------------------------------------------------ rule 6
def occupied_set(E, occupied_at, base=None):
    """indicator (float64 0 / 1) of {E >= occupied_at} united with the base occupancy (> 0.75) when given"""
    occ = E >= int(occupied_at)
    if base is not None:
        occ = occ | (np.asarray(base) > 0.75)
    return occ.astype(np.float64)


def field_of(oracle, E, occupied_at, cell, base=None):
    return mr.field_of(oracle, occupied_set(E, occupied_at, base), cell)


# ------------------------------------------------------------------------------------------------ whole calls
def integrate_points(E, n, origin, cell, sensor_origin, points, opts=None, centers=None, radii=None, margin=0.0,
                     batch=False):
    """What gpmp2mi_sdf_integrate_points must leave: (E', stats dict)"""
    opts = options() if opts is None else opts
    cls, a, b, _ = classify(n, origin, cell, sensor_origin, points, None, None, centers, radii, margin)
    miss, hit = (marks_of_batch if batch else marks_of)(n, cls, a, b)
    E2 = apply(E, miss, hit, opts)
    return E2, stats_of(cls, E2, opts)


def integrate_depth(E, n, origin, cell, cam, depth, opts=None, centers=None, radii=None, margin=0.0, batch=False):
    """What gpmp2mi_sdf_integrate_depth must leave: (E', stats dict)"""
    opts = options() if opts is None else opts
    z = np.asarray(depth, dtype=np.float32).astype(np.float64).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        p = deproject(cam, z)
    cls, a, b, _ = classify(n, origin, cell, camera_origin(cam), p, z, cam, centers, radii, margin)
    miss, hit = (marks_of_batch if batch else marks_of)(n, cls, a, b)
    E2 = apply(E, miss, hit, opts)
    return E2, stats_of(cls, E2, opts)
