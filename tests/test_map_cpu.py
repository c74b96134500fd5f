"""The numpy reference of the live map (tests/map_reference.py) pinned by literals, without a GPU: the point-to-cell rule
at the half-cell faces, the order of the classification, the stats, and the field of a one-point cloud.  The GPU tests
(tests/test_gpu_map.py) compare the device against this reference bit for bit."""
import numpy as np

import map_reference as mr


def test_one_point_in_a_row_of_five_gives_the_known_field(oracle):
    # nx = 5, ny = 1, cell 0.1, origin 0: the point 0.2 has u = 2.5 -> cell 2
    field, stats, occ = mr.update_from_points(oracle, (5, 1), [0.0, 0.0], 0.1, [[0.2, 0.0]])
    assert occ.tolist() == [[0.0, 0.0, 1.0, 0.0, 0.0]]
    assert stats == dict(kept=1, non_finite=0, self=0, outside=0)
    np.testing.assert_array_equal(field, np.array([[0.2, 0.1, -0.1, 0.1, 0.2]]))


def test_the_lower_half_cell_face_is_inside_and_the_upper_one_outside():
    n, origin, cell = (4, 3), [1.0, -2.0], 0.25
    lo = 1.0 - 0.125                                  # u = -0.5 + 0.5 = 0 exactly: kept, cell 0
    below = np.nextafter(lo, -np.inf)                 # u just below 0: outside
    hi = 1.0 + (4 - 0.5) * 0.25                       # u = n: outside
    under_hi = np.nextafter(hi, -np.inf)              # u just below n: kept, cell n - 1
    pts = np.array([[lo, -2.0], [below, -2.0], [hi, -2.0], [under_hi, -2.0], [1.0, -2.0 - 0.125], [1.0, -2.0 + 2.5 * 0.25]])
    u = mr.cell_coordinate(pts, origin, cell)
    assert u[0, 0] == 0.0 and u[1, 0] < 0.0 and u[2, 0] == 4.0 and u[3, 0] < 4.0 and u[4, 1] == 0.0 and u[5, 1] == 3.0
    cls, idx = mr.classify(pts, n, origin, cell)
    assert cls.tolist() == [mr.KEPT, mr.OUTSIDE, mr.OUTSIDE, mr.KEPT, mr.KEPT, mr.OUTSIDE]
    assert idx[0].tolist() == [0, 0] and idx[3].tolist() == [3, 0] and idx[4].tolist() == [0, 0]


def test_the_verdict_at_the_lower_face_is_the_comparison_of_u_for_any_cell_size():
    # -0.5 + 0.5 is exact; whether the next double below the face is outside is decided by u < 0 in double, nothing else
    for cell in (0.1, 0.01, 0.05, 1.0 / 3.0):
        p = np.array([[np.nextafter(-0.5 * cell, -np.inf)], [-0.5 * cell]])
        p = np.concatenate([p, np.zeros((2, 1))], axis=1)
        cls, _ = mr.classify(p, (3, 3), [0.0, 0.0], cell)
        u = mr.cell_coordinate(p, [0.0, 0.0], cell)
        assert cls[1] == mr.KEPT and u[1, 0] == 0.0, cell
        assert (cls[0] == mr.OUTSIDE) == bool(u[0, 0] < 0.0), cell    # the verdict is the comparison of u, nothing else


def test_the_first_matching_rule_applies_and_the_stats_sum_to_m():
    centers, radii = np.array([[0.5, 0.5, 0.5]]), np.array([0.2])
    nan, inf = np.nan, np.inf
    pts = np.array([[0.5, 0.5, nan],        # inside the sphere in x, y and NaN in z: non-finite comes first
                    [0.5, 0.5, 0.5],        # self
                    [0.5, 0.5, 0.7],        # on the boundary: <= counts as self
                    [0.5, 0.5, 0.75],       # kept
                    [9.0, 0.5, 0.5],        # outside
                    [-inf, 0.5, 0.5],       # non-finite, not outside
                    [0.5, 0.5, 0.74]])      # self only with the margin
    cls, _ = mr.classify(pts, (10, 10, 10), [0.0, 0.0, 0.0], 0.1, centers, radii, 0.0)
    assert cls.tolist() == [mr.NON_FINITE, mr.SELF, mr.SELF, mr.KEPT, mr.OUTSIDE, mr.NON_FINITE, mr.KEPT]
    st = mr.stats_of(cls)
    assert st == dict(kept=2, non_finite=2, self=2, outside=1) and sum(st.values()) == len(pts)
    cls, _ = mr.classify(pts, (10, 10, 10), [0.0, 0.0, 0.0], 0.1, centers, radii, 0.05)
    assert cls.tolist()[-1] == mr.SELF and sum(mr.stats_of(cls).values()) == len(pts)
    # a sphere outside the grid: a point in it is self, not outside
    cls, _ = mr.classify([[5.0, 5.0, 5.0]], (10, 10, 10), [0.0, 0.0, 0.0], 0.1, [[5.0, 5.0, 5.1]], [0.2])
    assert cls.tolist() == [mr.SELF]


def test_planar_points_use_x_and_y_of_the_centres_only():
    cls, _ = mr.classify([[0.3, 0.4]], (10, 10), [0.0, 0.0], 0.1, [[0.0, 0.0, 7.0]], [0.5])
    assert cls.tolist() == [mr.SELF]           # sqrt(0.09 + 0.16) = 0.5 <= 0.5, whatever z of the centre says
    cls, _ = mr.classify([[0.3, 0.41]], (10, 10), [0.0, 0.0], 0.1, [[0.0, 0.0, 7.0]], [0.5])
    assert cls.tolist() == [mr.KEPT]


def test_empty_and_full_sets_give_the_constant_and_the_base_is_united(oracle):
    n, origin, cell = (4, 3, 2), [0.0, 0.0, 0.0], 0.5
    field, stats, _ = mr.update_from_points(oracle, n, origin, cell, np.zeros((0, 3)))
    assert field.shape == (2, 3, 4) and (field == 1000.0).all() and sum(stats.values()) == 0
    every = np.array([[x, y, z] for z in range(2) for y in range(3) for x in range(4)]) * cell
    field, stats, occ = mr.update_from_points(oracle, n, origin, cell, every)
    assert occ.all() and (field == 1000.0).all() and stats["kept"] == 24
    base = np.zeros((2, 3, 4))
    base[1, 2, 3] = 1.0
    _, _, occ = mr.update_from_points(oracle, n, origin, cell, [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]], base=base)
    assert occ.sum() == 2 and occ[0, 0, 0] == 1.0 and occ[1, 2, 3] == 1.0       # duplicates mark one cell


def test_the_boundary_band_of_random_clouds_is_negligible(oracle):
    """The GPU test drops the points within 1e-9 of a sphere boundary before it compares verdicts; with the clouds it
    draws (tests/map_cases.py self_cloud) that is far below 1 % of them."""
    import map_cases as g
    for setup in ("wam", "point2d"):
        centers, radii, lo, hi = g.self_setup_cpu(oracle, setup)
        for margin in (0.0, 0.05):
            pts = g.self_cloud(centers, radii, lo, hi, seed=7)
            band = mr.boundary_band(pts, centers, radii, margin)
            assert band.sum() <= 0.01 * len(pts), (setup, margin, int(band.sum()))
