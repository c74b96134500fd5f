"""Sensor map on the device (include/gpmp2mi.h "sensor map"): evidence kept on a field handle, raised where rays end and
lowered where they pass, against the reference of tests/sensor_reference.py.  Every comparison is exact
(assert_array_equal): the evidence as int16, the stats as integers, the field bit for bit."""
import ctypes as C

import numpy as np
import pytest

import map_cases as mc
import map_reference as mr
import sensor_cases as sc
import sensor_reference as sr
from gpmp2_amd import engine as E, problems

pytestmark = pytest.mark.gpu


def _fresh(engine, n, value=0.25):
    origin, cell = sc.geometry(n)
    return engine.sdf(origin, cell, np.full(mr.grid_shape(n), value)), origin, cell


def _field(engine, s):
    return engine.sdf_field(s)["data"]


def _check(engine, oracle, s, E_want, stats, stats_want, cell, occupied_at=1, base=None, msg=""):
    print(msg, stats)
    assert stats == stats_want, (msg, stats, stats_want)
    np.testing.assert_array_equal(engine.sdf_evidence(s), E_want, err_msg=msg)
    np.testing.assert_array_equal(_field(engine, s), sr.field_of(oracle, E_want, occupied_at, cell, base), err_msg=msg)


@pytest.fixture(scope="module")
def point_frames(oracle):
    """{(n, which): (sensor origin, points, E after one frame on zero evidence, stats)}: the reference, computed once"""
    out = {}
    for n in (sc.GRID_3D, sc.GRID_2D):
        origin, cell = sc.geometry(n)
        for which in ("inside", "outside"):
            o, pts = sc.points_frame(n, which)
            E1, st = sr.integrate_points(np.zeros(mr.grid_shape(n), dtype=np.int16), n, origin, cell, o, pts)
            out[n, which] = (o, pts, E1, st)
    return out


# ---------------------------------------------------------------------------------------------- 1. points form, 2. order
@pytest.mark.parametrize("which", ["inside", "outside"])
@pytest.mark.parametrize("n", [sc.GRID_3D, sc.GRID_2D], ids=str)
def test_points_form_evidence_stats_and_field_equal_the_reference(engine, oracle, point_frames, n, which):
    s, origin, cell = _fresh(engine, n)
    o, pts, E1, want = point_frames[n, which]
    assert (engine.sdf_evidence(s) == 0).all()                       # before the first call: all 0, nothing allocated
    stats = engine.sdf_integrate_points(s, pts, o)
    assert sum(stats[c] for c in sr.STAT_NAMES[:5]) == len(pts)
    assert min(stats[c] for c in ("hit", "invalid", "outside")) > 0 and stats["invalid"] >= 4 and stats["occupied"] > 0
    _check(engine, oracle, s, E1, stats, want, cell, msg=f"{n} {which} frame 1")
    assert (E1 < 0).any() and (E1 > 0).any()
    # M = 0 leaves the evidence alone
    stats = engine.sdf_integrate_points(s, np.zeros((0, len(n))), o)
    assert stats == dict(hit=0, invalid=0, max_range=0, self=0, outside=0, occupied=want["occupied"])
    np.testing.assert_array_equal(engine.sdf_evidence(s), E1)
    # the same rays in another order, on top: the same evidence, stats and field as the reference's second frame
    E2, want2 = sr.integrate_points(E1, n, origin, cell, o, pts)
    perm = np.random.default_rng(5).permutation(len(pts))
    stats = engine.sdf_integrate_points(s, pts[perm], o)
    _check(engine, oracle, s, E2, stats, want2, cell, msg=f"{n} {which} frame 2, permuted")
    # and from zero again, permuted, against the first frame
    engine.sdf_evidence_reset(s)
    assert (engine.sdf_evidence(s) == 0).all()
    stats = engine.sdf_integrate_points(s, pts[perm[::-1]], o)
    _check(engine, oracle, s, E1, stats, want, cell, msg=f"{n} {which} frame 1, permuted")


def test_a_non_finite_sensor_origin_is_refused(engine):
    s, origin, cell = _fresh(engine, sc.GRID_2D)
    before = _field(engine, s)
    for bad in ([np.nan, 0.0], [0.0, np.inf]):
        with pytest.raises(E.Gpmp2miError) as ei:
            engine.sdf_integrate_points(s, np.zeros((3, 2)), bad)
        assert ei.value.code == 1 and "sensor_origin" in str(ei.value)
    np.testing.assert_array_equal(_field(engine, s), before)
    assert (engine.sdf_evidence(s) == 0).all()


# ---------------------------------------------------------------------------------------------- 3. depth form
@pytest.fixture(scope="module")
def wall_frames():
    """the reference on the (24, 20, 16) grid: E after the wall image with its bad pixels, its stats, and the classes"""
    n, cam = sc.GRID_3D, sc.camera()
    origin, cell = sc.geometry(n)
    z = sc.wall_image_with_bad_pixels()
    E1, st = sr.integrate_depth(np.zeros(mr.grid_shape(n), dtype=np.int16), n, origin, cell, cam, z)
    return cam, z, E1, st


def test_depth_form_equals_the_reference_and_the_points_form(engine, oracle, wall_frames):
    n = sc.GRID_3D
    cam, z, E1, want = wall_frames
    s, origin, cell = _fresh(engine, n)
    stats = engine.sdf_integrate_depth(s, cam, z)
    assert stats["hit"] > 500 and stats["invalid"] == 5 and stats["max_range"] == 2 and stats["self"] == 0
    _check(engine, oracle, s, E1, stats, want, cell, msg="wall with bad pixels")
    # the max_range rays carve and mark nothing at their end: an image of nothing but such pixels leaves no positive cell
    engine.sdf_evidence_reset(s)
    far = np.full_like(z, 4.0)
    E_far, want_far = sr.integrate_depth(np.zeros_like(E1), n, origin, cell, cam, far)
    stats = engine.sdf_integrate_depth(s, cam, far)
    assert stats["max_range"] == far.size and stats["occupied"] == 0
    _check(engine, oracle, s, E_far, stats, want_far, cell, msg="all beyond depth_max")
    assert (E_far <= 0).all() and (E_far < 0).sum() > 100 and (_field(engine, s) == 1000.0).all()
    # the reference's points, fed to the points form with the camera's origin, give the same evidence.  (A pixel beyond
    # depth_max has no counterpart in the points form: it is made invalid on both sides.)
    zp = z.copy()
    zp[zp > cam["depth_max"]] = np.nan
    pts = sr.deproject(cam, zp.astype(np.float64).reshape(-1))
    pts[~(zp.reshape(-1) >= cam["depth_min"])] = np.nan
    a, b = _fresh(engine, n)[0], _fresh(engine, n)[0]
    st_a = engine.sdf_integrate_depth(a, cam, zp)
    st_b = engine.sdf_integrate_points(b, pts, sr.camera_origin(cam))
    assert st_a == st_b and st_a["max_range"] == 0 and st_a["invalid"] == 7
    np.testing.assert_array_equal(engine.sdf_evidence(a), engine.sdf_evidence(b))
    np.testing.assert_array_equal(_field(engine, a), _field(engine, b))


# ---------------------------------------------------------------------------------------------- 4. evidence over frames
def test_evidence_over_frames_clamps_and_clears(engine, oracle):
    n, cam = sc.GRID_3D, sc.camera()
    s, origin, cell = _fresh(engine, n)
    opts = dict(hit=2, miss=1, lo=-2, hi=5, occupied_at=3)
    ro = sr.options(**opts)
    wall, behind = sc.wall_image(0.6), sc.wall_image(1.0)             # the second image sees through where the wall was
    Eref = np.zeros(mr.grid_shape(n), dtype=np.int16)
    wall_cells = None
    cleared_at = None
    for k, z in enumerate([wall] * 3 + [behind] * 4):
        Eref, want = sr.integrate_depth(Eref, n, origin, cell, cam, z, ro)
        stats = engine.sdf_integrate_depth(s, cam, z, **opts)
        _check(engine, oracle, s, Eref, stats, want, cell, occupied_at=3, msg=f"frame {k}")
        if k == 1:
            wall_cells = Eref == 4
            assert wall_cells.sum() > 50
        if k == 2:
            assert (Eref[wall_cells] == 5).all() and Eref.max() == 5  # 2, 4, then the clamp at hi
        if k > 2 and cleared_at is None and (Eref[wall_cells] < 3).all():
            cleared_at = k
    assert cleared_at == 5                                            # 5 -> 4 -> 3 -> 2: the third frame without the wall
    assert Eref.min() == -2                                           # and the clamp at lo
    # refresh = 0 changes the evidence and not the field; the rebuild alone then gives it
    before = _field(engine, s)
    Eref, want = sr.integrate_depth(Eref, n, origin, cell, cam, wall, ro)
    stats = engine.sdf_integrate_depth(s, cam, wall, refresh=False, **opts)
    assert stats == want
    np.testing.assert_array_equal(engine.sdf_evidence(s), Eref)
    np.testing.assert_array_equal(_field(engine, s), before)
    for occupied_at in (1, 3):
        engine.sdf_refresh_from_evidence(s, occupied_at)
        np.testing.assert_array_equal(_field(engine, s), sr.field_of(oracle, Eref, occupied_at, cell))
        np.testing.assert_array_equal(engine.sdf_evidence(s), Eref)  # the rebuild leaves the evidence alone
    # the live map's calls neither read nor change the evidence
    engine.sdf_update(s, before)
    engine.sdf_update_from_points(s, mc.cloud(n, origin, cell, 65, 3), use_base=False)
    engine.sdf_update_from_occupancy(s, mc.random_occupancy(n, seed=2))
    np.testing.assert_array_equal(engine.sdf_evidence(s), Eref)
    # nothing at or above the threshold: the empty set
    engine.sdf_refresh_from_evidence(s, 6)
    assert (_field(engine, s) == 1000.0).all()
    engine.sdf_evidence_reset(s)
    assert (engine.sdf_evidence(s) == 0).all()
    assert (_field(engine, s) == 1000.0).all()                        # a reset leaves the field alone


# ---------------------------------------------------------------------------------------------- 5. base
@pytest.mark.parametrize("n", [sc.GRID_3D, sc.GRID_2D], ids=str)
def test_base_is_united_with_the_evidence_and_cannot_be_cleared(engine, oracle, point_frames, n):
    s, origin, cell = _fresh(engine, n)
    o, pts, E1, want = point_frames[n, "inside"]
    before = _field(engine, s)
    with pytest.raises(E.Gpmp2miError) as ei:                         # no base yet
        engine.sdf_integrate_points(s, pts, o, use_base=True)
    assert ei.value.code == 1 and "base" in str(ei.value)
    with pytest.raises(E.Gpmp2miError) as ei:
        engine.sdf_refresh_from_evidence(s, 1, use_base=True)
    assert ei.value.code == 1 and "base" in str(ei.value)
    np.testing.assert_array_equal(_field(engine, s), before)          # a refused call changes nothing
    assert (engine.sdf_evidence(s) == 0).all()
    occ = mc.random_occupancy(n, seed=3, p=0.08)
    engine.sdf_update_from_occupancy(s, occ)
    stats = engine.sdf_integrate_points(s, pts, o, use_base=True)
    _check(engine, oracle, s, E1, stats, want, cell, base=occ, msg=f"{n} with base")
    carved = (E1 < 0) & (occ > 0.75)
    assert carved.sum() > 0                                           # rays went through base cells: lower evidence there,
    assert (_field(engine, s)[carved] <= 0.0).all()                   # and still obstacles
    stats = engine.sdf_integrate_points(s, pts, o, use_base=False)    # the same frame again, without the base
    E2, want2 = sr.integrate_points(E1, n, origin, cell, o, pts)
    _check(engine, oracle, s, E2, stats, want2, cell, msg=f"{n} without base")
    engine.sdf_refresh_from_evidence(s, 1, use_base=True)             # the base is still there
    np.testing.assert_array_equal(_field(engine, s), sr.field_of(oracle, E2, 1, cell, occ))


# ---------------------------------------------------------------------------------------------- 6. self filter
@pytest.mark.parametrize("margin", [0.0, 0.05])
@pytest.mark.parametrize("setup", ["wam", "point2d"])
def test_self_rays_carve_and_do_not_mark(engine, oracle, setup, margin):
    g = mc.self_setup(setup)
    r, s = engine.robot(g["model"]), engine.sdf(g["origin"], g["cell"], g["data"])
    centers = engine.sphere_centers(r, g["conf"])[0][0]               # the device's own bits: no point is left out
    radii = np.asarray(g["model"].flat()["sphere_radius"], dtype=np.float64)
    o_grid, nn = np.asarray(g["origin"], dtype=np.float64), np.asarray(g["n"], dtype=np.float64)
    lo, hi = o_grid - 0.5 * g["cell"], o_grid + (nn - 0.5) * g["cell"]
    pts = mc.self_cloud(centers, radii, lo, hi, seed=7, per_sphere=12, uniform=150)
    sensor = lo + 0.9 * (hi - lo)                                     # in a corner of the grid, away from the body
    E0 = np.zeros(mr.grid_shape(g["n"]), dtype=np.int16)
    E1, want = sr.integrate_points(E0, g["n"], g["origin"], g["cell"], sensor, pts, None, centers, radii, margin)
    stats = engine.sdf_integrate_points(s, pts, sensor, robot=r, conf=g["conf"], margin=margin)
    assert stats["self"] > 0 and stats["hit"] > 0
    _check(engine, oracle, s, E1, stats, want, g["cell"], msg=f"{setup} margin {margin}")
    # without the filter the same rays mark their ends: more hits, no self
    E2, want2 = sr.integrate_points(E0, g["n"], g["origin"], g["cell"], sensor, pts)
    engine.sdf_evidence_reset(s)
    stats2 = engine.sdf_integrate_points(s, pts, sensor)
    _check(engine, oracle, s, E2, stats2, want2, g["cell"], msg=f"{setup} no filter")
    assert stats2["self"] == 0 and stats2["hit"] > stats["hit"] and (E2 > 0).sum() > (E1 > 0).sum()
    assert stats2["hit"] + stats2["outside"] == stats["hit"] + stats["outside"] + stats["self"]


def test_planner_field_classes_integrate_on_the_live_handle_and_keep_data_in_step(oracle, wall_frames, point_frames):
    from gpmp2_amd import planner as P
    cam, z, E1, want = wall_frames
    n = sc.GRID_3D
    origin, cell = sc.geometry(n)
    f3 = P.SignedDistanceField(origin, cell, n[1], n[0], n[2])
    for k in range(n[2]):
        f3.initFieldData(k, np.full((n[1], n[0]), 0.5))
    h = f3.handle()
    assert f3.integrateDepth(cam, z) == want and f3.handle() is h     # the same handle: planners on it see the change
    np.testing.assert_array_equal(f3.evidence(), E1)
    np.testing.assert_array_equal(f3.raw_data(), sr.field_of(oracle, E1, 1, cell))
    o, pts, _, _ = point_frames[n, "inside"]
    E2, want2 = sr.integrate_points(E1, n, origin, cell, o, pts)
    assert f3.integratePoints(pts, o) == want2
    np.testing.assert_array_equal(f3.raw_data(), sr.field_of(oracle, E2, 1, cell))
    f3.refreshFromEvidence(4)
    np.testing.assert_array_equal(f3.raw_data(), sr.field_of(oracle, E2, 4, cell))
    f3.resetEvidence()
    assert (f3.evidence() == 0).all()
    n2 = sc.GRID_2D
    origin2, cell2 = sc.geometry(n2)
    f2 = P.PlanarSDF(origin2, cell2, np.full(mr.grid_shape(n2), 0.5))
    o, pts, E1, want = point_frames[n2, "outside"]
    assert f2.integratePoints(pts, o, hit=2) == want
    np.testing.assert_array_equal(f2.evidence(), E1)
    np.testing.assert_array_equal(f2.raw_data(), sr.field_of(oracle, E1, 1, cell2))


# ---------------------------------------------------------------------------------------------- 7. plans see it
def test_a_plan_made_before_an_integrate_call_sees_the_new_map(engine, oracle):
    p = problems.wam_restarts(B=3, total_step=10, obs_check_inter=2, opt="GN", sdf="40")
    n, cell = (40, 40, 40), float(p.sdf_cell)
    occ_a = (np.asarray(p.sdf_data) < 0.0).astype(np.float64)
    mid = 0.5 * (problems.WAM_START + problems.WAM_END)
    hand = oracle.sphere_centers(oracle.robot(p.model), mid)[0][0][-1]
    k = np.arange(-2, 3) * cell
    box = np.array([[hand[0] + dx, hand[1] + dy, hand[2] + dz] for dz in k for dy in k for dx in k])
    sensor = np.asarray(p.sdf_origin, dtype=np.float64) + 3.0 * cell
    r = engine.robot(p.model)
    s = engine.sdf(p.sdf_origin, p.sdf_cell, np.zeros((40, 40, 40)))
    engine.sdf_update_from_occupancy(s, occ_a)

    def solve(pl):
        pl.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
        err0 = pl.graph_error(p.init)
        pl.optimize()
        res = pl.result()
        return dict(err0=err0, iters=res["iters"], final_error=res["final_error"], traj=res["traj"], score=pl.score(2))

    pl = engine.plan(r, s, p.setting, p.B)
    on_a = solve(pl)
    stats = engine.sdf_integrate_points(s, box, sensor, use_base=True)
    E1, want = sr.integrate_points(np.zeros((40, 40, 40), dtype=np.int16), n, p.sdf_origin, cell, sensor, box)
    assert stats == want and stats["hit"] == len(box)
    np.testing.assert_array_equal(engine.sdf_evidence(s), E1)
    on_b = solve(pl)
    fresh = engine.sdf_from_occupancy(p.sdf_origin, p.sdf_cell, sr.occupied_set(E1, 1, occ_a))
    pf = engine.plan(r, fresh, p.setting, p.B)
    want_b = solve(pf)
    for key in ("err0", "iters", "final_error", "traj"):
        np.testing.assert_array_equal(on_b[key], want_b[key], err_msg=key)
    for key in on_b["score"]:
        np.testing.assert_array_equal(on_b["score"][key], want_b["score"][key], err_msg="score " + key)
    assert not np.array_equal(on_a["err0"], on_b["err0"])
    rng = np.random.default_rng(8)
    o = np.asarray(p.sdf_origin)
    q = rng.uniform(o - 2 * cell, o + 41 * cell, size=(400, 3))       # some out of range
    for got, ref in zip(engine.sdf_query(s, q), engine.sdf_query(fresh, q)):
        np.testing.assert_array_equal(got, ref)
    # 8. lifetime: the handle goes with its evidence workspace allocated, after the plans on it
    pf.close()
    pl.close()
    fresh.close()
    s.close()
    r.close()


# ---------------------------------------------------------------------------------------------- _dev forms
_DEV = r"""
import numpy as np
import torch                      # torch's HIP runtime first, as bench.py does
torch.cuda.init()
import sys
sys.path.insert(0, "tests")
import map_cases as mc
import sensor_cases as sc
from gpmp2_amd import engine as E
eng = E.Engine()
n, cam = sc.GRID_3D, sc.camera()
origin, cell = sc.geometry(n)
g = mc.self_setup("wam")
r = eng.robot(g["model"])
data = np.full(n[::-1], 0.25)
host, dev_ = eng.sdf(origin, cell, data), eng.sdf(origin, cell, data)
occ = mc.random_occupancy(n, seed=21, p=0.02)
o, pts = sc.points_frame(n, "inside")
z = sc.wall_image_with_bad_pixels()
opts = dict(hit=3, miss=1, lo=-3, hi=7, occupied_at=2)
dev = torch.device("cuda:0")
traj = torch.zeros(11, 14, dtype=torch.float64, device=dev)
traj[3, :7] = torch.from_numpy(g["conf"]).to(dev)
conf_ptr = traj.data_ptr() + 3 * 14 * 8        # the configuration of support state 3, inside the trajectory tensor
t_occ, t_pts, t_z = torch.from_numpy(occ).to(dev), torch.from_numpy(pts).to(dev), torch.from_numpy(z).to(dev)
t_stats = [torch.full((6,), -7, dtype=torch.int32, device=dev) for _ in range(3)]
eng.sdf_reserve_update(dev_)
eng.sdf_reserve_evidence(dev_)
torch.cuda.synchronize()
st = torch.cuda.Stream(device=dev)
# the base, a frame of points, two depth frames (the second one evidence only), then the rebuild: one stream, no host
# synchronisation in between
eng.sdf_update_from_occupancy_dev(dev_, t_occ, stream=st.cuda_stream)
eng.sdf_integrate_points_dev(dev_, len(pts), t_pts, o, r, conf_ptr, 0.02, t_stats[0], stream=st.cuda_stream, use_base=True, **opts)
eng.sdf_integrate_depth_dev(dev_, cam, t_z, r, conf_ptr, 0.02, t_stats[1], stream=st.cuda_stream, use_base=True, **opts)
eng.sdf_integrate_depth_dev(dev_, cam, t_z, stats=t_stats[2], stream=st.cuda_stream, refresh=False, **opts)
eng.sdf_refresh_from_evidence(dev_, 4, True, stream=st.cuda_stream, dev=True)
st.synchronize()
eng.sdf_update_from_occupancy(host, occ)
want = [eng.sdf_integrate_points(host, pts, o, r, g["conf"], 0.02, use_base=True, **opts),
        eng.sdf_integrate_depth(host, cam, z, r, g["conf"], 0.02, use_base=True, **opts),
        eng.sdf_integrate_depth(host, cam, z, refresh=False, **opts)]
eng.sdf_refresh_from_evidence(host, 4, True)
for s, w in zip(t_stats, want):
    assert s.cpu().numpy().tolist() == [w[k] for k in E.Engine.EVIDENCE_STATS], (s, w)
assert want[0]["hit"] > 0 and want[1]["hit"] > 0 and want[1]["max_range"] == 2
bits = lambda a: np.ascontiguousarray(a).view(np.int64)
assert np.array_equal(eng.sdf_evidence(dev_), eng.sdf_evidence(host)) and eng.sdf_evidence(host).max() >= 6
assert np.array_equal(bits(eng.sdf_field(dev_)["data"]), bits(eng.sdf_field(host)["data"]))
eng.sdf_evidence_reset(dev_, stream=st.cuda_stream, dev=True)
st.synchronize()
assert (eng.sdf_evidence(dev_) == 0).all()
try:
    eng.sdf_update_dev(dev_, torch.from_numpy(data).to(dev), stream=st.cuda_stream)       # a plain update clears the base
    eng.sdf_integrate_depth_dev(dev_, cam, t_z, stream=st.cuda_stream, use_base=True)
    raise SystemExit("use_base without a base was accepted")
except E.Gpmp2miError as e:
    assert e.code == 1
print("SENSOR DEV OK")
"""


def test_dev_forms_equal_the_host_calls_bit_for_bit():
    """the `_dev` forms from torch tensors on a torch stream, back to back after sdf_reserve_evidence; in a fresh process
    that starts torch's HIP runtime before the library, as bench.py does"""
    import importlib.util
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert importlib.util.find_spec("torch") is not None    # not imported here: this process keeps the library's runtime
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root] + [x for x in [os.environ.get("PYTHONPATH")] if x]))
    r = subprocess.run([sys.executable, "-c", _DEV], capture_output=True, text=True, timeout=300, cwd=root, env=env)
    assert r.returncode == 0 and "SENSOR DEV OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------------------------------------- 8. refusals on a device
def test_refusals_that_need_a_device(engine, wall_frames):
    cam, z, _, _ = wall_frames
    planar, origin, cell = _fresh(engine, sc.GRID_2D)
    before = _field(engine, planar)
    c, o = E.Engine._camera(cam), E.Engine._evidence_opts({})
    rc = engine.lib.gpmp2mi_sdf_integrate_depth(planar.ptr, C.byref(c), z.ctypes.data_as(C.POINTER(C.c_float)), None,
                                                None, 0.0, C.byref(o), None)
    assert rc == 1 and "3-D" in engine.lib.gpmp2mi_last_error().decode()
    np.testing.assert_array_equal(_field(engine, planar), before)
    assert (engine.sdf_evidence(planar) == 0).all()
    # reserve, then destroy a handle that never integrated anything
    engine.sdf_reserve_evidence(planar)
    assert (engine.sdf_evidence(planar) == 0).all()
    planar.close()
    if engine.device_count() >= 2:                                    # a robot on another device than the field
        hip = C.CDLL("libamdhip64.so")
        g = mc.self_setup("wam")
        s = engine.sdf(g["origin"], g["cell"], g["data"])
        assert hip.hipSetDevice(1) == 0
        try:
            r = engine.robot(g["model"])
        finally:
            assert hip.hipSetDevice(0) == 0
        with pytest.raises(E.Gpmp2miError) as ei:
            engine.sdf_integrate_points(s, np.zeros((4, 3)), np.asarray(g["origin"]), robot=r, conf=g["conf"])
        assert ei.value.code == 1 and "another device" in str(ei.value)
        assert (engine.sdf_evidence(s) == 0).all()
