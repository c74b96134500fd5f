"""Inputs of the sensor-map tests (tests/test_gpu_sensor.py, tests/test_sensor_cpu.py): the two grids, ray sets given in
cell coordinates with their edge cases, and the depth camera with its planted wall.  Pure numpy and seeded, so the CPU
and the GPU tests see the same rays."""
import numpy as np

import map_reference as mr

GRID_3D, GRID_2D = (24, 20, 16), (13, 10)      # (nx, ny(, nz)): unequal, so a swapped axis shows
IMAGE = (32, 24)                               # width, height


def geometry(n):
    """(origin, cell): the grid straddles the world's origin on every axis.  A world point p has cell coordinates
    (p - origin) / cell + 0.5; the difference is exact but only as fine as the larger of |p| and |origin|, so a
    lattice value is hit bit for bit only where |p| is small against |p - origin|: the upper three quarters of this
    grid."""
    return [-0.6, -0.5, -0.4][:len(n)], 0.05


def world_point(u, origin, cell, exact=True):
    """A world point whose cell coordinates (p - origin) / cell + 0.5 are `u`; with exact, bit for bit: the doubles
    around origin + (u - 0.5) cell are searched for one that maps back to u exactly, and None is returned when there is
    none."""
    u = np.asarray(u, dtype=np.float64)
    o = np.asarray(origin, dtype=np.float64)[:len(u)]
    p = o + (u - 0.5) * cell
    if not exact:
        return p
    for k in range(len(u)):
        for cand in _neighbours(p[k], 16):
            if (cand - o[k]) / cell + 0.5 == u[k]:
                p[k] = cand
                break
        else:
            return None
    return p


def _neighbours(x, steps):
    yield x
    lo = hi = x
    for _ in range(steps):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        yield lo
        yield hi


def sensor_origins(n):
    """{name: cell coordinates of the sensor}: inside the grid on a cell face in x and at cell centres otherwise; and at a
    cell centre three cells outside the high x face"""
    origin, cell = geometry(n)

    def reachable(k, values):                              # the first value on axis k that some double maps to exactly
        for v in values:
            u = np.full(len(n), 0.5)
            u[k] = v
            p = world_point(u, origin, cell)
            if p is not None:
                return v
        raise AssertionError((k, values))

    centres = [[7.5, 6.5, 8.5, 5.5, 9.5], [5.5, 4.5, 6.5, 3.5, 7.5]]
    inside = [reachable(0, [10.0, 11.0, 9.0, 12.0])] + [reachable(k, centres[k - 1]) for k in range(1, len(n))]
    beyond = [n[0] + 2.0 + f for f in (0.5, 0.25, 0.75, 0.125, 0.375, 0.625, 0.875)]
    outside = [reachable(0, beyond)] + [reachable(k, centres[k - 1][::-1]) for k in range(1, len(n))]
    return dict(inside=np.array(inside), outside=np.array(outside))


def ray_ends(n, a, seed):
    """End points of a frame in cell coordinates [M][dim], as (exact [Me][dim], loose [Ml][dim], bad [Mb][dim]): exact ones
    must be hit bit for bit in cell coordinates (lattice and half-lattice values), loose ones are random, bad ones hold
    NaN / inf world coordinates.  Every class but self occurs; see the comments for the edge cases."""
    dim = len(n)
    rng = np.random.default_rng(seed)
    nn = np.asarray(n, dtype=np.float64)
    a = np.asarray(a, dtype=np.float64)
    exact = []
    e = np.eye(dim)
    for k in range(dim):                                   # parallel to an axis, both ways, inside and leaving the grid
        for m in (1.0, 4.0, -3.0, -6.0, nn[k] + 4.0):
            exact.append(a + m * e[k])
    for signs in ([1, 1, 1], [1, -1, 1], [-1, 1, -1], [1, 1, -1], [0, 1, 1], [0, -1, 1], [1, 0, 1], [1, 1, 0]):
        for m in (1.0, 3.0, 4.0):                          # exact diagonals: equal t on the moving axes (the tie rule)
            exact.append(a + m * np.asarray(signs[:dim], dtype=np.float64))
    for _ in range(24):                                    # ends exactly on cell faces (lattice points) and half-way
        exact.append(np.floor(rng.uniform(0.0, nn)))
        exact.append(np.floor(rng.uniform(0.0, nn)) + 0.5)
    exact.append(a.copy())                                 # left = 0: the single cell
    exact.append(a.copy())                                 # a duplicate
    exact.append(np.zeros(dim))                            # the lowest corner of the grid
    exact.append(nn.copy())                                # the first lattice point beyond it on every axis: outside
    loose = [rng.uniform(-3.0, nn + 3.0) for _ in range(120)]
    far = a.copy()
    far[0] += 2.0e6                                        # invalid by the span rule
    far[1] += 1.0
    loose.append(far)
    far = a.copy()
    far[0] += 1.0e5                                        # outside, and the walk must return
    far[1] += 3.0e4
    loose.append(far)
    bad = []
    for v in (np.nan, np.inf, -np.inf):
        q = a + 1.0
        q[dim - 1] = v
        bad.append(q)
    return np.array(exact), np.array(loose), np.array(bad)


def points_frame(n, which, seed=1):
    """(sensor_origin [dim], points [M][dim]) in the world for the grid n and the sensor 'inside' / 'outside'"""
    origin, cell = geometry(n)
    a = sensor_origins(n)[which]
    o = world_point(a, origin, cell)
    assert o is not None, a
    exact, loose, bad = ray_ends(n, a, seed)
    pts = [world_point(u, origin, cell) for u in exact]
    keep = [p is not None for p in pts]                    # what no double reaches is left out; the CPU test counts the rest
    exact, pts = exact[keep], [p for p in pts if p is not None]
    pts += [world_point(u, origin, cell, exact=False) for u in loose]
    for u in bad:                                          # NaN / inf stay what they are in the world
        p = world_point(np.where(np.isfinite(u), u, 0.0), origin, cell, exact=False)
        pts.append(np.where(np.isfinite(u), p, u))
    pts = np.array(pts)
    assert (mr.cell_coordinate(o[None, :], origin, cell)[0] == a).all()
    assert (mr.cell_coordinate(pts[:len(exact)], origin, cell) == exact).all()
    return o, pts


# ------------------------------------------------------------------------------------------------ depth
def _rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def camera(depth_min=0.1, depth_max=2.0):
    """32 x 24 pinhole camera inside the (24, 20, 16) grid, rotated about y and then x: its optical axis points along
    (0.74, 0.48, 0.47), so the three axes of the grid are told apart"""
    w, h = IMAGE
    R = _rot(1, 1.0) @ _rot(0, -0.5)
    pose = np.concatenate([R, np.array([[-0.4], [-0.3], [-0.25]])], axis=1)
    return dict(width=w, height=h, fx=30.0, fy=30.0, cx=15.5, cy=11.5, depth_min=depth_min, depth_max=depth_max, pose=pose)


def wall_image(depth=0.6):
    """a wall square to the optical axis at `depth` metres"""
    w, h = IMAGE
    return np.full((h, w), depth, dtype=np.float32)


BAD_PIXELS = {(2, 3): np.nan, (5, 7): np.inf, (9, 11): 0.0, (12, 20): -1.0, (15, 25): 0.05, (18, 6): 3.0, (20, 30): 7.5}


def wall_image_with_bad_pixels():
    """the wall, and single pixels (row, column) that are NaN, +inf, 0, negative, below depth_min and above depth_max"""
    z = wall_image()
    for (v, u), value in BAD_PIXELS.items():
        z[v, u] = value
    return z
