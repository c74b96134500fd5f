"""Scene on the device (include/gpmp2mi.h "scene"): boxes, spheres, cylinders and closed meshes rasterised against the
reference of tests/scene_reference.py, and the field rebuilt from them.  Every comparison is exact: masks byte for byte,
counts entry for entry, fields bit for bit."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import map_cases as mc
import map_reference as mr
import scene_cases as sc
import scene_reference as sr
from gpmp2_amd import engine as E, problems

pytestmark = pytest.mark.gpu

MAIN = "33x20x16"
GENERAL_CUBE = ((-0.212, -0.113, -0.071), (0.318, 0.287, 0.333))
INFLATE = sc.CELL_MAIN * np.sqrt(3.0) / 2.0


def _torus_at(t):
    return sc.mesh(sc.torus(), sc.pose(sc.rotation((1.0, 0.4, 0.2), 0.9), t))


def _mixed(grid):
    """every kind around the middle of a grid, sized by its sides; the torus reaches over the grid's faces in y"""
    n, origin, cell = sc.GRIDS[grid]
    c = sc.centre_of(n, origin, cell)
    u = cell * max(2.0, min(0.25 * n[1], n[0] / 16.0))
    scale = lambda vt, f: (vt[0] * f, vt[1])
    return [sc.box([1.5 * u, 0.6 * u, 0.8 * u], sc.pose(sc.R_GENERAL, c + [-3 * u, 0.5 * u, 0.0])),
            sc.sphere(0.9 * u, c + [2.5 * u, -0.7 * u, 0.3 * cell]),
            sc.cylinder(0.7 * u, 1.2 * u, sc.pose(sc.rotation((0.2, 1.0, 0.1), 1.1), c + [0.3 * u, 0.9 * u, 0.0]), inflate=0.4 * cell),
            sc.mesh(scale(sc.icosphere(), u / 0.17), sc.pose(t=c + [5 * u, 0.2 * u, 0.1 * cell])),
            sc.mesh(scale(sc.torus(), 4 * u), sc.pose(sc.rotation((1.0, 0.4, 0.2), 0.5), c + [-1.0 * u, -0.4 * u, 0.2 * cell])),
            sc.mesh(scale(sc.tetrahedron(), 4 * u), sc.pose(sc.R_GENERAL, c + [-6 * u, 0.0, 0.0]))]


CASES = {                                     # name -> (grid, objects)
    "box": lambda: (MAIN, [sc.box([0.21, 0.12, 0.08], sc.pose(sc.R_GENERAL, (0.2, 0.15, 0.2)))]),
    "box inflated": lambda: (MAIN, [sc.box([0.21, 0.12, 0.08], sc.pose(sc.R_GENERAL, (0.2, 0.15, 0.2)), inflate=INFLATE)]),
    "sphere": lambda: (MAIN, [sc.sphere(0.19, (0.31, 0.12, 0.17))]),
    "sphere inflated": lambda: (MAIN, [sc.sphere(0.19, (0.31, 0.12, 0.17), inflate=INFLATE)]),
    "cylinder": lambda: (MAIN, [sc.cylinder(0.11, 0.23, sc.pose(sc.R_GENERAL, (0.3, 0.2, 0.15)))]),
    "cylinder inflated": lambda: (MAIN, [sc.cylinder(0.11, 0.23, sc.pose(sc.R_GENERAL, (0.3, 0.2, 0.15)), inflate=INFLATE)]),
    "sphere without a centre": lambda: (MAIN, [sc.sphere(0.3 * sc.CELL_MAIN, np.asarray(sc.ORIGIN_MAIN) + 5.5 * sc.CELL_MAIN)]),
    "general cube": lambda: (MAIN, [sc.mesh(sc.cube(*GENERAL_CUBE))]),
    "lattice cube": lambda: (MAIN, [sc.mesh(sc.lattice_cube())]),
    "tetrahedron": lambda: (MAIN, [sc.mesh(sc.tetrahedron(), sc.pose(sc.R_GENERAL, (0.25, 0.15, 0.2)))]),
    "icosphere": lambda: (MAIN, [sc.mesh(sc.icosphere(), sc.pose(sc.R_GENERAL, (0.3, 0.17, 0.18)))]),
    "torus -x": lambda: (MAIN, [sc.mesh(sc.torus(), sc.TORUS_POSE_MAIN)]),
    "torus +x": lambda: (MAIN, [_torus_at((1.05, 0.18, 0.18))]),
    "torus -y": lambda: (MAIN, [_torus_at((0.3, -0.25, 0.18))]),
    "torus +y": lambda: (MAIN, [_torus_at((0.3, 0.6, 0.18))]),
    "torus -z": lambda: (MAIN, [_torus_at((0.3, 0.18, -0.15))]),
    "torus +z": lambda: (MAIN, [_torus_at((0.3, 0.18, 0.5))]),
    "two overlapping meshes": lambda: (MAIN, [sc.mesh(sc.cube((-0.2, -0.1, 0.0), (0.2, 0.2, 0.3))),
                                              sc.mesh(sc.cube((0.0, 0.0, 0.1), (0.4, 0.3, 0.4)))]),
    "mesh wholly outside": lambda: (MAIN, [sc.mesh(sc.icosphere(), sc.pose(t=(3.0, 0.2, 0.2))), sc.sphere(0.1, (0.2, 0.2, 0.2))]),
    "disabled object": lambda: (MAIN, [sc.box([0.2, 0.1, 0.1], sc.pose(t=(0.2, 0.2, 0.2)), enabled=False),
                                       sc.mesh(sc.lattice_cube(), enabled=False), sc.sphere(0.12, (0.6, 0.2, 0.2))]),
    "mesh out of range": lambda: (MAIN, [sc.mesh(sc.icosphere(), sc.pose(t=(2.0 ** 19 * sc.CELL_MAIN, 0.0, 0.0))),
                                         sc.mesh(sc.tetrahedron(), sc.pose(t=(0.3, 0.2, 0.2)))]),
    "mixed 64x5x3": lambda: ("64x5x3", _mixed("64x5x3")),
    "mixed 70x9x1": lambda: ("70x9x1", _mixed("70x9x1")),
    "mixed planar": lambda: ("40x30", _mixed("40x30")),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(grid, objects, reference mask, reference cells): computed once"""
    grid, objs = CASES[name]()
    n, origin, cell = sc.GRIDS[grid]
    mask, cells = sr.rasterize(objs, n, origin, cell)
    return grid, objs, mask, cells


def _rasterize(scene, grid):
    n, origin, cell = sc.GRIDS[grid]
    return scene.rasterize(origin, cell, mr.grid_shape(n))


def _field(engine, s):
    return engine.sdf_field(s)["data"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------------------------------------- 1. rasterize
@pytest.mark.parametrize("name", list(CASES))
def test_rasterize_equals_the_reference_byte_for_byte(engine, name):
    grid, objs, want, want_cells = _case(name)
    scene = engine.scene(objs)
    mask, cells = _rasterize(scene, grid)
    print(name, cells.tolist(), int(mask.sum()))
    assert cells.tolist() == want_cells
    np.testing.assert_array_equal(mask, want)
    again, cells2 = _rasterize(scene, grid)              # the bit volume was left clear: the same bytes again
    np.testing.assert_array_equal(again, want)
    assert cells2.tolist() == want_cells
    scene.close()


def test_known_answers_and_edge_cases_are_what_the_cases_claim():
    """the reference side of the cases above says what they are meant to say (no GPU work here beyond the fixture)"""
    assert _case("general cube")[3] == [704] and _case("lattice cube")[3] == [216]
    lattice = np.zeros(mr.grid_shape(sc.GRID_MAIN), dtype=np.uint8)
    lattice[2:8, 4:10, 4:10] = 1
    np.testing.assert_array_equal(_case("lattice cube")[2], lattice)
    assert _case("sphere without a centre")[3] == [0]
    assert _case("mesh wholly outside")[3][0] == 0 and _case("mesh wholly outside")[3][1] > 0
    assert _case("disabled object")[3][:2] == [0, 0] and _case("disabled object")[3][2] > 0
    assert _case("mesh out of range")[3][0] == -1 and _case("mesh out of range")[3][1] > 0
    assert len(sc.icosphere()[1]) == 320
    for kind in ("box", "sphere", "cylinder"):
        assert 0 < _case(kind)[3][0] < _case(kind + " inflated")[3][0]
    a, b = _case("two overlapping meshes")[3]
    assert _case("two overlapping meshes")[2].sum() < a + b
    faces = {"-x": (2, 0), "+x": (2, -1), "-y": (1, 0), "+y": (1, -1), "-z": (0, 0), "+z": (0, -1)}
    for f, (axis, idx) in faces.items():
        m = _case("torus " + f)[2]
        assert np.take(m, idx, axis=axis).any(), f       # cut by that face
        assert 100 < m.sum() < 395
    for name in ("mixed 64x5x3", "mixed 70x9x1", "mixed planar"):
        assert min(_case(name)[3]) > 0, (name, _case(name)[3])


def test_set_poses_set_enabled_and_shuffled_triangles(engine):
    grid, objs, want, want_cells = _case("torus -x")
    v, t = sc.torus()
    scene = engine.scene([sc.mesh((v, sc.shuffled(t)), sc.TORUS_POSE_MAIN), sc.sphere(0.1, (0.6, 0.2, 0.2), enabled=False)])
    mask, cells = _rasterize(scene, grid)
    np.testing.assert_array_equal(mask, want)            # the triangle list shuffled: the same bytes
    assert cells.tolist() == want_cells + [0]
    # the torus moves to the +y face and the sphere is switched on: the scene made there in the first place
    moved = _torus_at((0.3, 0.6, 0.18))
    scene.set_poses([moved["pose"]], first=0)
    scene.set_enabled([True], first=1)
    want2, want_cells2 = sr.rasterize([moved, sc.sphere(0.1, (0.6, 0.2, 0.2))], *sc.GRIDS[grid])
    mask, cells = _rasterize(scene, grid)
    np.testing.assert_array_equal(mask, want2)
    assert cells.tolist() == want_cells2 and want_cells2[0] == _case("torus +y")[3][0]
    # refusals that need a live handle change nothing
    for call in (lambda: scene.engine.lib.gpmp2mi_scene_set_poses(scene.ptr, 1, 2, E.dptr(np.zeros(24))),
                 lambda: scene.engine.lib.gpmp2mi_scene_set_poses(scene.ptr, -1, 1, E.dptr(np.zeros(12))),
                 lambda: scene.engine.lib.gpmp2mi_scene_set_poses(scene.ptr, 0, 1, E.dptr(np.full(12, np.nan))),
                 lambda: scene.engine.lib.gpmp2mi_scene_set_poses(scene.ptr, 0, 1, None),
                 lambda: scene.engine.lib.gpmp2mi_scene_set_enabled(scene.ptr, 2, 1, E.iptr(np.zeros(1, dtype=np.int32)))):
        assert call() == 1
    assert engine.lib.gpmp2mi_scene_count(scene.ptr) == 2
    np.testing.assert_array_equal(_rasterize(scene, grid)[0], want2)
    scene.close()


# ---------------------------------------------------------------------------------------------- 2. the field
@pytest.mark.parametrize("grid", [MAIN, "40x30"])
def test_update_from_scene_equals_the_occupancy_constructor_bit_for_bit(engine, grid):
    n, origin, cell = sc.GRIDS[grid]
    shape = mr.grid_shape(n)
    objs = _case("two overlapping meshes")[1] + _case("cylinder")[1] if grid == MAIN else _mixed(grid)
    want_mask, want_cells = sr.rasterize(objs, n, origin, cell)
    scene = engine.scene(objs)
    s = engine.sdf(origin, cell, np.full(shape, 0.25))
    before = _field(engine, s)
    # refusals that need a live handle: no base and no evidence yet
    for kw, word in ((dict(use_base=True), "base"), (dict(use_evidence=True), "evidence")):
        with pytest.raises(E.Gpmp2miError) as ei:
            engine.sdf_update_from_scene(s, scene, **kw)
        assert ei.value.code == 1 and word in str(ei.value)
    np.testing.assert_array_equal(_field(engine, s), before)
    # the base and the evidence come from earlier calls on the same handle
    occ = mc.random_occupancy(n, seed=5, p=0.01)
    engine.sdf_update_from_occupancy(s, occ)
    c = sc.centre_of(n, origin, cell)[:len(n)]
    rng = np.random.default_rng(6)
    lo = np.asarray(origin, dtype=np.float64)
    pts = rng.uniform(lo, lo + (np.asarray(n) - 1) * cell, size=(60, len(n)))
    for _ in range(2):
        engine.sdf_integrate_points(s, pts, c, refresh=False)
    Eh = engine.sdf_evidence(s)
    assert (Eh >= 3).sum() > 10 and (occ > 0.75).sum() > 3
    rq = rng.uniform(lo - 2 * cell, lo + (np.asarray(n) + 1) * cell, size=(300, len(n)))
    for use_base in (False, True):
        for use_evidence in (False, True):
            cells = engine.sdf_update_from_scene(s, scene, use_base, use_evidence, occupied_at=3)
            assert cells.tolist() == want_cells
            O = sr.occupied_set(want_mask, occ if use_base else None, Eh if use_evidence else None, 3)
            fresh = engine.sdf_from_occupancy(origin, cell, O)
            msg = f"{grid} base {use_base} evidence {use_evidence}"
            assert np.array_equal(_bits(_field(engine, s)), _bits(_field(engine, fresh))), msg
            for got, ref in zip(engine.sdf_query(s, rq), engine.sdf_query(fresh, rq)):        # the packed cells
                np.testing.assert_array_equal(got, ref, err_msg=msg)
            fresh.close()
            np.testing.assert_array_equal(engine.sdf_evidence(s), Eh, err_msg=msg)             # E is unchanged
    # the base is unchanged: an update from no points with the base gives the field of the base alone
    engine.sdf_update_from_points(s, np.zeros((0, len(n))), use_base=True)
    fresh = engine.sdf_from_occupancy(origin, cell, occ)
    assert np.array_equal(_bits(_field(engine, s)), _bits(_field(engine, fresh)))
    # nothing occupied: the constant 1000
    scene.set_enabled([False] * len(objs))
    assert engine.sdf_update_from_scene(s, scene).tolist() == [0] * len(objs)
    assert (_field(engine, s) == 1000.0).all()
    for h in (fresh, s, scene):
        h.close()


def test_planner_field_classes_update_from_a_scene(engine):
    from gpmp2_amd import planner as P
    from gpmp2_amd import scene as S
    grid, objs, want, want_cells = _case("lattice cube")
    n, origin, cell = sc.GRIDS[grid]
    f3 = P.SignedDistanceField(origin, cell, n[1], n[0], n[2])
    for k in range(n[2]):
        f3.initFieldData(k, np.full((n[1], n[0]), 0.5))
    h = f3.handle()
    cube = objs[0]
    cells = f3.update_from_scene(S.Scene([S.Mesh(cube["vertices"], cube["triangles"])]))
    assert cells.tolist() == [216] and f3.handle() is h
    fresh = engine.sdf_from_occupancy(origin, cell, want.astype(np.float64))
    assert np.array_equal(_bits(f3.raw_data()), _bits(_field(engine, fresh)))
    n2, origin2, cell2 = sc.GRIDS["40x30"]
    f2 = P.PlanarSDF(origin2, cell2, np.full(mr.grid_shape(n2), 0.5))
    disc = [S.Sphere(0.2, (0.0, 0.0, 0.0)), S.Box([0.05, 0.3, 1.0], S.pose_of(t=(0.2, 0.0, 0.0)))]
    cells = f2.update_from_scene(disc)
    want2, want_cells2 = sr.rasterize([sc.sphere(0.2, (0, 0, 0)), sc.box([0.05, 0.3, 1.0], sc.pose(t=(0.2, 0, 0)))], n2, origin2, cell2)
    assert cells.tolist() == want_cells2
    fresh2 = engine.sdf_from_occupancy(origin2, cell2, want2.astype(np.float64))
    assert np.array_equal(_bits(f2.raw_data()), _bits(_field(engine, fresh2)))


# ---------------------------------------------------------------------------------------------- 3. plans see it
def test_a_plan_made_before_the_update_sees_the_new_box(engine, oracle):
    p = problems.wam_restarts(B=3, total_step=10, obs_check_inter=2, opt="GN", sdf="40")
    n, cell = (40, 40, 40), float(p.sdf_cell)
    mid = 0.5 * (problems.WAM_START + problems.WAM_END)
    hand = oracle.sphere_centers(oracle.robot(p.model), mid)[0][0][-1]
    r = engine.robot(p.model)
    s = engine.sdf(p.sdf_origin, p.sdf_cell, np.full((40, 40, 40), 1000.0))      # the empty map
    pl = engine.plan(r, s, p.setting, p.B)
    pl.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
    err_free = pl.graph_error(p.init)
    half = 2.0 * cell
    obj = sc.box([half, half, half], sc.pose(sc.rotation((0.0, 0.0, 1.0), 0.4), hand))
    scene = engine.scene([obj])
    cells = engine.sdf_update_from_scene(s, scene)
    want_mask, want_cells = sr.rasterize([obj], n, p.sdf_origin, cell)
    assert cells.tolist() == want_cells and want_cells[0] > 30
    err_box = pl.graph_error(p.init)
    print("straight line: free", err_free[0], "through the box", err_box[0])
    assert err_box[0] > err_free[0]                      # row 0 is the straight line, and it runs through the box
    pl.optimize()
    res, score = pl.result(), pl.score(2)
    print("final_error", res["final_error"], "min_clearance", score["min_clearance"])
    assert score["min_clearance"].max() > 0.0             # (parts of the arm leave this small map: out_of_range is not 0)
    # and it is the plan a fresh field of the same obstacle set gives
    fresh = engine.sdf_from_occupancy(p.sdf_origin, p.sdf_cell, want_mask.astype(np.float64))
    pf = engine.plan(r, fresh, p.setting, p.B)
    pf.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
    np.testing.assert_array_equal(pf.graph_error(p.init), err_box)
    pf.optimize()
    np.testing.assert_array_equal(pf.result()["traj"], res["traj"])
    for h in (pf, pl, fresh, s, scene, r):
        h.close()


# ---------------------------------------------------------------------------------------------- 4. _dev forms
class _DevArray:
    """a device buffer from the library's own HIP runtime (gpmp2mi_debug_device_*): no second runtime in the process"""

    def __init__(self, engine, shape, dtype, fill_byte=0x7B):
        self.eng, self.host = engine, np.zeros(shape, dtype=dtype)
        self.p = C.c_void_p()
        engine._ck(engine.lib.gpmp2mi_debug_device_alloc(C.c_size_t(self.host.nbytes), fill_byte, C.byref(self.p)))

    @property
    def ptr(self):
        return self.p.value

    def read(self):
        self.eng._ck(self.eng.lib.gpmp2mi_debug_device_read(self.host.ctypes.data_as(C.c_void_p), self.p,
                                                            C.c_size_t(self.host.nbytes)))
        return self.host.copy()

    def free(self):
        self.eng._ck(self.eng.lib.gpmp2mi_debug_device_free(self.p))


def test_dev_forms_on_a_callers_stream_equal_the_host_forms(engine):
    lib = engine.lib
    n, origin, cell = sc.GRIDS[MAIN]
    shape = mr.grid_shape(n)
    objs = _case("torus -x")[1] + _case("box")[1] + _case("mesh out of range")[1][:1]
    want_mask, want_cells = sr.rasterize(objs, n, origin, cell)
    scene = engine.scene(objs)
    host, dev = (engine.sdf(origin, cell, np.full(shape, 0.25)) for _ in range(2))
    occ = mc.random_occupancy(n, seed=7, p=0.01)
    for s in (host, dev):
        engine.sdf_update_from_occupancy(s, occ)
    scene.reserve(shape)                                  # from here on the `_dev` forms neither allocate nor wait
    d_mask, d_cells, d_cells2 = _DevArray(engine, shape, np.uint8), _DevArray(engine, (3,), np.int32), _DevArray(engine, (3,), np.int32)
    st, tok = C.c_void_p(), C.c_void_p()
    engine._ck(lib.gpmp2mi_debug_stream_create(C.byref(st)))
    engine._ck(lib.gpmp2mi_debug_stall_begin(st, 3000, C.byref(tok)))            # parks the stream, 3 s at the most
    try:
        t0 = time.perf_counter()
        engine.scene_rasterize_dev(scene, origin, cell, shape, d_mask.ptr, d_cells.ptr, stream=st.value)
        engine.sdf_update_from_scene_dev(dev, scene, use_base=True, cells=d_cells2.ptr, stream=st.value)
        took = time.perf_counter() - t0
    finally:
        engine._ck(lib.gpmp2mi_debug_stall_release(tok))  # releases the stall and waits for that stream
    assert took < 1.0, ("a `_dev` call waited for its stream", took)
    np.testing.assert_array_equal(d_mask.read(), want_mask)
    assert d_cells.read().tolist() == want_cells and d_cells2.read().tolist() == want_cells and want_cells[2] == -1
    cells = engine.sdf_update_from_scene(host, scene, use_base=True)
    assert cells.tolist() == want_cells
    assert np.array_equal(_bits(_field(engine, dev)), _bits(_field(engine, host)))
    fresh = engine.sdf_from_occupancy(origin, cell, sr.occupied_set(want_mask, occ))
    assert np.array_equal(_bits(_field(engine, dev)), _bits(_field(engine, fresh)))
    engine._ck(lib.gpmp2mi_debug_stream_destroy(st))
    for b in (d_mask, d_cells, d_cells2):
        b.free()
    for h in (fresh, host, dev, scene):
        h.close()
