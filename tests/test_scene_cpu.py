"""The mesh rule of include/gpmp2mi.h "scene" without a GPU: the known answers of the numpy reference
(tests/scene_reference.py), its invariances, and the product's own text of the integer rule (gpmp2_amd/csrc/scene_rule.h,
built by g++ through tests/scene_shim.py) against the reference's Python integers."""
import numpy as np
import pytest

import scene_cases as sc
import scene_reference as sr
import scene_shim

N, ORIGIN, CELL = sc.GRID_MAIN, sc.ORIGIN_MAIN, sc.CELL_MAIN


def _centres():
    cx, cy, cz = sr.cell_centres(N, ORIGIN, CELL)
    return np.stack(np.broadcast_arrays(cx[None, None, :], cy[None, :, None], cz[:, None, None]), axis=-1)


def test_general_cube_is_the_interval_box_of_cell_centres():
    lo, hi = np.array([-0.212, -0.113, -0.071]), np.array([0.318, 0.287, 0.333])
    m = sr.mesh_mask(*sc.cube(lo, hi), sc.pose(), N, ORIGIN, CELL)
    c = _centres()
    want = ((c >= lo) & (c <= hi)).all(axis=-1)
    assert m.sum() == 704 and want.sum() == 704
    np.testing.assert_array_equal(m, want)


def test_lattice_cube_shows_the_tie_rule():
    m = sr.mesh_mask(*sc.lattice_cube(), sc.pose(), N, ORIGIN, CELL)
    want = np.zeros_like(m)
    want[2:8, 4:10, 4:10] = True                 # z 2..7, y 4..9, x 4..9: each face belongs to one side
    assert m.sum() == 216
    np.testing.assert_array_equal(m, want)


@pytest.mark.parametrize("which", ["general", "lattice", "torus"])
def test_triangle_order_and_winding_do_not_matter(which):
    v, t = {"general": lambda: sc.cube((-0.212, -0.113, -0.071), (0.318, 0.287, 0.333)), "lattice": sc.lattice_cube,
            "torus": sc.torus}[which]()
    P = sc.TORUS_POSE_MAIN if which == "torus" else sc.pose()
    m = sr.mesh_mask(v, t, P, N, ORIGIN, CELL)
    for seed in (1, 2):
        np.testing.assert_array_equal(sr.mesh_mask(v, sc.shuffled(t, seed), P, N, ORIGIN, CELL), m)
    np.testing.assert_array_equal(sr.mesh_mask(v, t[:, ::-1], P, N, ORIGIN, CELL), m)      # inside out


def test_torus_cut_by_the_low_x_face_stays_inside_the_analytic_torus_and_closes_its_rows():
    P = sc.TORUS_POSE_MAIN
    m = sr.mesh_mask(*sc.torus(), P, N, ORIGIN, CELL)
    d = sc.torus_distance(_centres(), P)
    sag = 0.006                                  # the facets leave the surface by at most 0.35 (1 - cos(pi / 24)) < 0.0031
    assert m.sum() > 200 and m[:, :, 0].any()    # it reaches the face it is cut by
    assert (d[m] < sag).all()                    # none outside the analytic torus
    assert m[d < -sag].all()                     # and nothing of its inside is missing
    assert not m[:, :, -1].any()                 # no row is left set at its +x end
    assert not m[:, :, 20:].any()


def test_two_overlapping_cubes_unite():
    a = sc.mesh(sc.cube((-0.2, -0.1, 0.0), (0.2, 0.2, 0.3)))
    b = sc.mesh(sc.cube((0.0, 0.0, 0.1), (0.4, 0.3, 0.4)))
    mask, cells = sr.rasterize([a, b], N, ORIGIN, CELL)
    ma, mb = sr.object_mask(a, N, ORIGIN, CELL)[0], sr.object_mask(b, N, ORIGIN, CELL)[0]
    assert (ma & mb).sum() > 20                  # they overlap, and the overlap stays occupied
    np.testing.assert_array_equal(mask.astype(bool), ma | mb)
    assert cells == [int(ma.sum()), int(mb.sum())] and mask.sum() < sum(cells)


def test_a_mesh_beyond_the_fixed_point_range_marks_nothing():
    far = 2.0 ** 19 * CELL                       # 2^19 cells: |g * 1024| reaches 2^29 there
    near = sc.mesh(sc.cube((-0.1, -0.1, -0.1), (0.1, 0.1, 0.1)))
    v, t = sc.cube((-0.1, -0.1, -0.1), (0.1, 0.1, 0.1))
    v = v.copy()
    v[7, 0] = ORIGIN[0] + far + CELL             # one vertex out of range takes the whole mesh with it
    mask, cells = sr.rasterize([near, sc.mesh((v, t))], N, ORIGIN, CELL)
    assert cells[1] == -1 and cells[0] > 0
    np.testing.assert_array_equal(mask.astype(bool), sr.object_mask(near, N, ORIGIN, CELL)[0])
    v[7, 0] = ORIGIN[0] + far - CELL             # just inside: a (huge) mesh again
    assert sr.rasterize([sc.mesh((v, t))], N, ORIGIN, CELL)[1][0] >= 0
    v[7, 0] = np.inf
    assert sr.rasterize([sc.mesh((v, t))], N, ORIGIN, CELL)[1] == [-1]


def test_a_sphere_that_holds_no_cell_centre_marks_nothing_and_the_inflate_of_the_header_covers():
    c = np.asarray(ORIGIN) + (np.array([5, 5, 5]) + 0.5) * CELL        # the corner between eight centres
    mask, cells = sr.rasterize([sc.sphere(0.3 * CELL, c)], N, ORIGIN, CELL)
    assert cells == [0] and not mask.any()
    mask, cells = sr.rasterize([sc.sphere(0.0, c, inflate=CELL * np.sqrt(3.0) / 2.0 * (1 + 1e-12))], N, ORIGIN, CELL)
    assert cells == [8]


# ---------------------------------------------------------------------------------------------- scene_rule.h through g++
def test_shim_quantize_is_the_reference():
    rng = np.random.default_rng(11)
    g = np.concatenate([rng.uniform(-600.0, 600.0, 300), (np.arange(-40, 40) + 0.5) / 1024.0,     # ties
                        [2.0 ** 19, -2.0 ** 19, np.nextafter(2.0 ** 19, 1e9), 1e300, np.inf, -np.inf, np.nan]])
    for x in g:
        s = np.float64(x) * 1024.0
        want = None if (not np.isfinite(x) or abs(s) > sr.FIXED_MAX) else int(np.rint(s))
        assert scene_shim.quantize(x) == want, x
    assert scene_shim.quantize(0.5 / 1024.0) == 0 and scene_shim.quantize(1.5 / 1024.0) == 2     # to even
    for v in list(range(-2050, 2050)) + [-2 ** 29, 2 ** 29]:
        assert scene_shim.floor_cell(v) == v // 1024 and scene_shim.ceil_cell(v) == -((-v) // 1024)


def _compare(P, Y, Z):
    got, extra = scene_shim.column(P, Y, Z)
    o = sr.orient(*P)
    if o is None:
        assert got == "skip"
        return "skip"
    assert got != "skip" and extra[1] == o[3]
    want = sr.column(*o, Y, Z)
    assert got == want, (P, Y, Z, got, want)
    return want


def test_shim_agrees_with_the_python_rule_on_random_integer_triangles():
    rng = np.random.default_rng(12)
    seen = {"skip": 0, "cross": 0, "miss": 0}
    for _ in range(1500):
        big = rng.integers(0, 2)
        lim = 2 ** 29 if big else 40 * 1024
        P = [[int(x) for x in rng.integers(-lim, lim + 1, 3)] for _ in range(3)]
        if rng.integers(0, 10) == 0:
            P[2] = [P[2][0]] + P[1][1:]          # a degenerate projection: a == 0
        for _ in range(6):
            w = rng.dirichlet(np.ones(3))        # columns near the triangle, and far from it
            Y = int(round(sum(w[k] * P[k][1] for k in range(3)) / 1024.0)) * 1024 if rng.integers(0, 4) else int(rng.integers(0, 64)) * 1024
            Z = int(round(sum(w[k] * P[k][2] for k in range(3)) / 1024.0)) * 1024
            r = _compare(P, Y, Z)
            seen["skip" if r == "skip" else ("miss" if r is None else "cross")] += 1
    assert min(seen.values()) > 50, seen


def test_shim_agrees_on_lattice_points_where_an_edge_function_is_zero():
    """vertices on cell centres: columns through vertices and along edges; each such point belongs to exactly one of the
    triangles around it, in the shim as in the reference"""
    rng = np.random.default_rng(13)
    zero = 0
    for _ in range(300):
        P = [[int(x) * 1024 for x in rng.integers(-6, 7, 3)] for _ in range(3)]
        for j in range(-6, 7):
            for k in range(-6, 7):
                r = _compare(P, 1024 * j, 1024 * k)
                if r != "skip":
                    e = scene_shim.column(P, 1024 * j, 1024 * k)[1][0]
                    zero += 0 in e
    assert zero > 2000
    # a fan of four triangles around the lattice point (2, 2): the column through it crosses exactly one of them
    c, ring = [0, 2048, 2048], [[0, 0, 0], [0, 4096, 0], [0, 4096, 4096], [0, 0, 4096]]
    hits = [scene_shim.column([c, ring[k], ring[(k + 1) % 4]], 2048, 2048)[0] for k in range(4)]
    assert sum(h is not None for h in hits) == 1
    assert hits == [sr.column(*sr.orient(c, ring[k], ring[(k + 1) % 4]), 2048, 2048) for k in range(4)]
    # and a column on the shared edge of two triangles crosses exactly one
    hits = [scene_shim.column(t, 1024, 1024)[0] for t in ([ring[0], ring[1], ring[2]], [ring[0], ring[2], ring[3]])]
    assert sum(h is not None for h in hits) == 1
