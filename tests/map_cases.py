"""Inputs of the live-map tests (tests/test_gpu_map.py, tests/test_map_cpu.py): the grids, the clouds with their edge
cases and the two self-filter setups.  Pure numpy and seeded, so the CPU and the GPU tests see the same points."""
import numpy as np

from gpmp2_amd import problems

GRIDS_3D = [(7, 5, 3), (33, 20, 9), (1, 8, 4), (40, 40, 40)]   # (nx, ny, nz)
GRIDS_2D = [(13, 10), (5, 1)]
CLOUD_SIZES = (0, 1, 63, 64, 65, 1000)                         # around one wavefront, and several workgroups


def geometry(n):
    """(origin, cell) of the test field with n cells per axis"""
    return [-0.35, 0.2, 0.1][:len(n)], 0.05


def cloud(n, origin, cell, M, seed):
    """M points [M][dim]: uniform over the grid's box grown by a cell on every side, and -- as far as M has room, from the
    back -- duplicates, points on half-cell faces (the lowest face of the grid included), one point beyond each face of
    the grid, NaN, +inf and -inf."""
    dim = len(n)
    rng = np.random.default_rng(seed)
    o, nn = np.asarray(origin, dtype=np.float64), np.asarray(n, dtype=np.float64)
    lo, hi = o - 1.5 * cell, o + (nn + 0.5) * cell
    p = rng.uniform(lo, hi, size=(M, dim))
    if M < 2:
        return p if M == 0 else o[None, :] + 0.0 * p           # one point: the centre of cell 0
    mid = o + np.floor(nn / 2) * cell                           # a cell centre inside
    special = [p[0], p[0], mid, mid]                            # duplicates
    for a in range(dim):
        for u in (-0.5, 0.5, n[a] - 0.5, n[a] - 1.5):           # the outer faces and the first inner ones
            q = mid.copy()
            q[a] = o[a] + u * cell
            special.append(q)
        for u in (-3.0, n[a] + 2.0):                            # beyond the two faces of this axis
            q = mid.copy()
            q[a] = o[a] + u * cell
            special.append(q)
    for bad in (np.nan, np.inf, -np.inf):
        q = mid.copy()
        q[dim - 1] = bad
        special.append(q)
    special = np.array(special)[:M - 1]
    p[M - len(special):] = special
    return p


def covering_cloud(n, origin, cell):
    """the centre of every cell, once"""
    axes = [np.arange(k, dtype=np.float64) for k in n]
    g = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, len(n))
    return np.asarray(origin)[None, :] + g * cell


def random_occupancy(n, seed, p=0.05):
    rng = np.random.default_rng(seed)
    return (rng.uniform(size=tuple(n)[::-1]) < p).astype(np.float64)


def self_setup(name):
    """dict(model, conf, n, origin, cell, data): 'wam' = the WAM arm at a non-zero configuration on the 40^3 desk field,
    'point2d' = the planar point robot of problems.point_robot_2d() on its own field"""
    if name == "wam":
        p = problems.wam_restarts(B=1, total_step=10, obs_check_inter=2, sdf="40")
        conf = problems.WAM_START.copy()
    else:
        p = problems.point_robot_2d()
        conf = np.array([-3.0, 4.0])
    data = np.asarray(p.sdf_data)
    return dict(model=p.model, conf=conf, n=data.shape[::-1], origin=list(p.sdf_origin), cell=float(p.sdf_cell), data=data)


def self_setup_cpu(oracle, name):
    """(oracle sphere centres [S][3], radii [S] in the caller's order, lo, hi of the grid's box)"""
    s = self_setup(name)
    centers = oracle.sphere_centers(oracle.robot(s["model"]), s["conf"])[0][0]
    radii = np.asarray(s["model"].flat()["sphere_radius"], dtype=np.float64)
    o = np.asarray(s["origin"], dtype=np.float64)
    return centers, radii, o - 0.5 * s["cell"], o + (np.asarray(s["n"]) - 0.5) * s["cell"]


def self_cloud(centers, radii, lo, hi, seed, per_sphere=40, uniform=400):
    """points around every sphere centre at 0 to 2 radii in random directions, plus uniform ones over the grid's box"""
    dim = len(lo)
    rng = np.random.default_rng(seed)
    parts = [rng.uniform(lo, hi, size=(uniform, dim))]
    for c, r in zip(np.asarray(centers), radii):
        d = rng.normal(size=(per_sphere, dim))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        parts.append(c[None, :dim] + d * (rng.uniform(0.0, 2.0, size=(per_sphere, 1)) * r))
    return np.concatenate(parts, axis=0)
