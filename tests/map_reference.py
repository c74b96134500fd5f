"""Numpy restatement of the rules of include/gpmp2mi.h "live map": the point-to-cell rule, the classification of a point
in its order, the self filter on given sphere centres, and the field of the occupied set through the oracle's distance
transform.  TEST INFRASTRUCTURE ONLY; every expression is written as the header writes it, in IEEE double."""
import numpy as np

KEPT, NON_FINITE, SELF, OUTSIDE = 0, 1, 2, 3
STAT_NAMES = ("kept", "non_finite", "self", "outside")


def grid_shape(n):
    """n = (nx, ny) or (nx, ny, nz) -> the array shape [ny][nx] or [nz][ny][nx]"""
    return tuple(int(x) for x in n)[::-1]


def cell_coordinate(points, origin, cell):
    """u = (p - origin) / cell + 0.5 per axis: a true division"""
    p = np.asarray(points, dtype=np.float64)
    return (p - np.asarray(origin, dtype=np.float64)[None, :p.shape[1]]) / np.float64(cell) + 0.5


def sphere_distance(points, centers):
    """[M][S] sqrt(dx^2 + dy^2 (+ dz^2)), summed in that order; planar points use x, y of the centres only"""
    p = np.asarray(points, dtype=np.float64)
    c = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
    dx, dy = p[:, None, 0] - c[None, :, 0], p[:, None, 1] - c[None, :, 1]
    d2 = dx * dx + dy * dy
    if p.shape[1] == 3:
        dz = p[:, None, 2] - c[None, :, 2]
        d2 = d2 + dz * dz
    return np.sqrt(d2)


def classify(points, n, origin, cell, centers=None, radii=None, margin=0.0):
    """-> (cls [M] of KEPT / NON_FINITE / SELF / OUTSIDE, idx [M][dim] cell indices (x, y(, z)), valid where kept).
    The first rule that matches applies: non-finite, self, outside, kept."""
    dim = len(n)
    p = np.asarray(points, dtype=np.float64).reshape(-1, dim)
    M = p.shape[0]
    cls = np.full(M, KEPT, dtype=np.int32)
    idx = np.zeros((M, dim), dtype=np.int64)
    finite = np.isfinite(p).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        inside_body = np.zeros(M, dtype=bool)
        if centers is not None and M:
            limit = np.asarray(radii, dtype=np.float64) + np.float64(margin)
            inside_body = (sphere_distance(p, centers) <= limit[None, :]).any(axis=1)
        u = cell_coordinate(p, origin, cell)
        in_grid = ((u >= 0.0) & (u < np.asarray(n, dtype=np.float64)[None, :])).all(axis=1)
    cls[~in_grid] = OUTSIDE
    cls[inside_body] = SELF
    cls[~finite] = NON_FINITE
    keep = cls == KEPT
    idx[keep] = np.floor(u[keep]).astype(np.int64)
    return cls, idx


def stats_of(cls):
    return {name: int((cls == k).sum()) for k, name in enumerate(STAT_NAMES)}


def occupied_set(n, cls, idx, base=None):
    """indicator [nz][ny][nx] / [ny][nx] (float64 0 / 1) of base united with the cells of the kept points"""
    occ = np.zeros(grid_shape(n)) if base is None else (np.asarray(base) > 0.75).astype(np.float64)
    k = idx[cls == KEPT]
    occ[tuple(k[:, a] for a in range(len(n) - 1, -1, -1))] = 1.0
    return occ


def field_of(oracle, occ, cell):
    """the oracle's field of an occupancy grid (1000 everywhere for an empty or a full one)"""
    return oracle.sdf_field_from_occupancy(np.ascontiguousarray(occ, dtype=np.float64), float(cell))


def update_from_points(oracle, n, origin, cell, points, base=None, centers=None, radii=None, margin=0.0):
    """What gpmp2mi_sdf_update_from_points must leave: (field, stats dict, occupied set)"""
    cls, idx = classify(points, n, origin, cell, centers, radii, margin)
    occ = occupied_set(n, cls, idx, base)
    return field_of(oracle, occ, cell), stats_of(cls), occ


def boundary_band(points, centers, radii, margin, width=1e-9):
    """[M] bool: the point lies within `width` of a sphere boundary radius + margin (its verdict could flip with the last
    bits of the centres); non-finite points are never in the band"""
    p = np.asarray(points, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = sphere_distance(p, centers) - (np.asarray(radii, dtype=np.float64) + np.float64(margin))[None, :]
        return (np.abs(d) <= width).any(axis=1)
