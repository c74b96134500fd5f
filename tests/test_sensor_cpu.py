"""The reference of the sensor map (tests/sensor_reference.py) pinned without a GPU: its voxel walk against a geometric
check that shares none of its arithmetic (every cell of a walk must meet the segment), three walks as literals, the apply
rule, the class order, and the inputs of tests/sensor_cases.py."""
import numpy as np
import pytest

import sensor_cases as sc
import sensor_reference as sr

N_RAYS = 20000


def _rays(dim, seed):
    """N_RAYS pairs (a, b) of cell coordinates in [-3, 27]: one sixth each general, starts on lattice points, ends on
    lattice points, one axis constant, exact diagonals from cell centres, half-integer end points"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-3.0, 27.0, size=(N_RAYS, dim))
    b = rng.uniform(-3.0, 27.0, size=(N_RAYS, dim))
    kind = np.arange(N_RAYS) % 6
    a[kind == 1] = np.floor(a[kind == 1])
    b[kind == 2] = np.floor(b[kind == 2])
    rows = np.flatnonzero(kind == 3)
    axis = rng.integers(0, dim, size=len(rows))
    b[rows, axis] = a[rows, axis]
    rows = np.flatnonzero(kind == 4)
    a[rows] = np.floor(a[rows]) + 0.5
    m = rng.integers(1, 12, size=(len(rows), 1)).astype(np.float64)
    b[rows] = a[rows] + m * rng.choice([-1.0, 1.0], size=(len(rows), dim))
    b[kind == 5] = np.floor(b[kind == 5]) + 0.5
    return a, b, kind


def _box_meets_segment(c, a, b, grow=1e-9):
    """slab clipping of the segment a -> b against the unit box of cell c grown by `grow`"""
    t0, t1 = 0.0, 1.0
    for k in range(len(c)):
        lo, hi, d = c[k] - grow, c[k] + 1.0 + grow, b[k] - a[k]
        if d == 0.0:
            if not lo <= a[k] <= hi:
                return False
            continue
        ta, tb = (lo - a[k]) / d, (hi - a[k]) / d
        t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
    return t0 <= t1 + 1e-12


@pytest.mark.parametrize("dim", [2, 3])
def test_every_cell_of_a_walk_meets_its_segment(dim):
    a, b, kind = _rays(dim, seed=40 + dim)
    assert all((kind == k).sum() >= N_RAYS // 6 for k in range(6))
    for i in range(N_RAYS):
        cells = sr.walk(a[i], b[i])
        assert cells[0] == tuple(int(x) for x in np.floor(a[i])) and cells[-1] == tuple(int(x) for x in np.floor(b[i])), i
        assert len(cells) == 1 + int(np.abs(np.floor(b[i]) - np.floor(a[i])).sum()), i
        for p, q in zip(cells, cells[1:]):
            assert sum(abs(x - y) for x, y in zip(p, q)) == 1, (i, p, q)
        for c in cells:
            assert _box_meets_segment(c, a[i], b[i]), (i, kind[i], c, a[i], b[i])


def test_three_walks_as_literals():
    cells = sr.walk([0.5, 0.5, 0.5], [3.5, 3.5, 3.5])          # every step a three-way tie: x, y, z, x, y, z, ...
    assert cells == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2), (3, 2, 2), (3, 3, 2), (3, 3, 3)]
    assert sr.walk([2.0, 1.5], [0.25, 1.5]) == [(2, 1), (1, 1), (0, 1)]       # a start on a face, going down
    assert sr.walk([4.25, 7.75, 1.5], [4.75, 7.25, 1.5]) == [(4, 7, 1)]       # left = 0: the single cell
    assert sr.walk([-0.5, 0.5], [0.5, -0.5]) == [(-1, 0), (0, 0), (0, -1)]    # a tie goes to x first, whatever the signs


def test_apply_rule_hit_wins_and_both_ends_clamp():
    opts = sr.options(hit=3, miss=2, lo=-3, hi=4)
    E = np.array([0, 0, 0, 3, -2, 4, -3], dtype=np.int16)
    miss = np.array([0, 1, 1, 0, 1, 0, 1], dtype=bool)
    hit = np.array([0, 0, 1, 1, 0, 1, 0], dtype=bool)
    out = sr.apply(E, miss, hit, opts)
    assert out.dtype == np.int16 and out.tolist() == [0, -2, 3, 4, -3, 4, -3]
    # evidence that an earlier call with wider limits left is clamped too
    assert sr.apply(np.array([9, -9], dtype=np.int16), np.zeros(2, bool), np.zeros(2, bool), opts).tolist() == [4, -3]


def test_marks_of_a_frame_carve_up_to_the_end_cell_only():
    n, origin, cell = (6, 4), [0.0, 0.0], 1.0
    # cell coordinates = world + 0.5; three rays from the centre of cell (0, 1): a hit at cell (4, 1), a ray that leaves
    # the grid, and a hit that ends in a cell the first ray passes
    o = np.array([0.0, 1.0])
    pts = np.array([[4.0, 1.0], [9.0, 1.0], [2.0, 1.0], [np.nan, 1.0]])
    cls, a, b, _ = sr.classify(n, origin, cell, o, pts)
    assert cls.tolist() == [sr.HIT, sr.OUTSIDE, sr.HIT, sr.INVALID]
    miss, hit = sr.marks_of(n, cls, a, b)
    assert miss[1].tolist() == [True] * 6 and not miss[[0, 2, 3]].any()        # the outside ray carves the whole row
    assert hit[1].tolist() == [False, False, True, False, True, False] and hit.sum() == 2
    E, stats = sr.integrate_points(np.zeros((4, 6), dtype=np.int16), n, origin, cell, o, pts)
    assert E[1].tolist() == [-1, -1, 2, -1, 2, -1]                              # a hit wins over the misses of other rays
    assert stats == dict(hit=2, invalid=1, max_range=0, self=0, outside=1, occupied=2)


def test_depth_classes_in_their_order():
    cam = sc.camera()
    n = sc.GRID_3D
    origin, cell = sc.geometry(n)
    z = sc.wall_image_with_bad_pixels().astype(np.float64).reshape(-1)
    cls, a, b, p = sr.classify(n, origin, cell, sr.camera_origin(cam), sr.deproject(cam, z), z, cam)
    w = cam["width"]
    want = {(2, 3): sr.INVALID, (5, 7): sr.INVALID, (9, 11): sr.INVALID, (12, 20): sr.INVALID, (15, 25): sr.INVALID,
            (18, 6): sr.MAX_RANGE, (20, 30): sr.MAX_RANGE}
    for (v, u), c in want.items():
        assert cls[v * w + u] == c, (v, u)
    assert (cls == sr.HIT).sum() > 500 and (cls == sr.INVALID).sum() == 5 and (cls == sr.MAX_RANGE).sum() == 2
    # a max_range ray ends where depth_max puts it: 2 m along the optical axis
    far = np.flatnonzero(cls == sr.MAX_RANGE)
    R = np.asarray(cam["pose"])[:, :3]
    np.testing.assert_allclose((p[far] - sr.camera_origin(cam)) @ R[:, 2], cam["depth_max"], rtol=1e-12)


@pytest.mark.parametrize("n", [sc.GRID_3D, sc.GRID_2D], ids=str)
@pytest.mark.parametrize("which", ["inside", "outside"])
def test_point_frames_hold_their_edge_cases(n, which):
    origin, cell = sc.geometry(n)
    o, pts = sc.points_frame(n, which)
    cls, a, b, _ = sr.classify(n, origin, cell, o, pts)
    counts = {name: int((cls == k).sum()) for k, name in enumerate(sr.STAT_NAMES[:5])}
    assert min(counts[c] for c in ("hit", "invalid", "outside")) > 0 and counts["invalid"] >= 4, counts
    d = b - a[None, :]
    with np.errstate(invalid="ignore"):
        assert ((np.abs(d) >= sr.MAX_SPAN).any(axis=1) & np.isfinite(pts).all(axis=1)).sum() == 1   # the span rule alone
        assert (cls[np.isfinite(d).all(axis=1) & (np.abs(d).max(axis=1) > 9.0e4)] != sr.HIT).all()
    # the frame keeps only the lattice values some double reaches (sensor_cases.geometry); enough of each kind are left
    lattice = (b == np.floor(b)).all(axis=1).sum()                                 # ends on lattice points
    moving = (d != 0) & np.isfinite(d)
    diagonal = ((np.abs(d) == np.abs(d[:, :1])) & moving).all(axis=1).sum()        # exact diagonals on every axis
    parallel = ((moving.sum(axis=1) == 1) & np.isfinite(d).all(axis=1)).sum()      # parallel to an axis
    print(n, which, counts, "lattice", lattice, "diagonal", diagonal, "parallel", parallel)
    assert lattice >= 6 and diagonal >= 4 and parallel >= 2 * len(n)


def test_batched_walk_gives_the_marks_of_the_ray_by_ray_walk():
    for dim in (2, 3):
        n = (sc.GRID_3D, sc.GRID_2D)[3 - dim]
        a, b, _ = _rays(dim, seed=50 + dim)
        for k in range(0, 3000, 500):                      # 500 rays from one start each, every special case among them
            cls = np.full(500, sr.OUTSIDE)
            cls[((b[k:k + 500] >= 0) & (b[k:k + 500] < np.asarray(n))).all(axis=1)] = sr.HIT
            cls[::17] = sr.INVALID
            want = sr.marks_of(n, cls, a[k], b[k:k + 500])
            got = sr.marks_of_batch(n, cls, a[k], b[k:k + 500])
            assert want[0].any() and want[1].any()
            np.testing.assert_array_equal(got[0], want[0])
            np.testing.assert_array_equal(got[1], want[1])
    n, cam = sc.GRID_3D, sc.camera()
    origin, cell = sc.geometry(n)
    E0 = np.zeros((16, 20, 24), dtype=np.int16)
    z = sc.wall_image_with_bad_pixels()
    one, st_one = sr.integrate_depth(E0, n, origin, cell, cam, z)
    two, st_two = sr.integrate_depth(E0, n, origin, cell, cam, z, batch=True)
    assert st_one == st_two
    np.testing.assert_array_equal(one, two)
