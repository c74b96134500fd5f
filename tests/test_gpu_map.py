"""Live map on the device (include/gpmp2mi.h "live map"): a field handle updated in place from a field, an occupancy grid
or a point cloud, against the numpy reference of tests/map_reference.py.  Fields and stats are compared bit for bit
(assert_array_equal, no tolerance), as the occupancy constructor is in test_sdf_from_occupancy_bit_exact."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import map_cases as mc
import map_reference as mr
from gpmp2_amd import engine as E, problems

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fresh(engine, n, value=0.25):
    origin, cell = mc.geometry(n)
    return engine.sdf(origin, cell, np.full(mr.grid_shape(n), value)), origin, cell


def _field(engine, s):
    return engine.sdf_field(s)["data"]


# ---------------------------------------------------------------------------------------------- 1. points only
@pytest.mark.parametrize("n", mc.GRIDS_3D + mc.GRIDS_2D, ids=str)
def test_points_only_field_and_stats_equal_the_reference(engine, oracle, n):
    s, origin, cell = _fresh(engine, n)
    for k, M in enumerate(mc.CLOUD_SIZES):
        pts = mc.cloud(n, origin, cell, M, seed=100 + k)
        want, want_stats, _ = mr.update_from_points(oracle, n, origin, cell, pts)
        stats = engine.sdf_update_from_points(s, pts, use_base=False)
        assert stats == want_stats and sum(stats.values()) == M, (M, stats, want_stats)
        np.testing.assert_array_equal(_field(engine, s), want, err_msg=f"M = {M}")
        if M == 0:
            assert (want == 1000.0).all()
        if M == 1000:
            assert min(want_stats[c] for c in ("kept", "non_finite", "outside")) > 0    # every class but self occurs
    # the same points in another order: the same field
    perm = np.random.default_rng(5).permutation(len(pts))
    engine.sdf_update_from_points(s, pts[perm], use_base=False)
    np.testing.assert_array_equal(_field(engine, s), want)
    # every cell covered: no free space left
    every = mc.covering_cloud(n, origin, cell)
    stats = engine.sdf_update_from_points(s, every, use_base=False)
    assert stats == dict(kept=len(every), non_finite=0, self=0, outside=0)
    assert (_field(engine, s) == 1000.0).all()


# ---------------------------------------------------------------------------------------------- 2. base
@pytest.mark.parametrize("n", [(33, 20, 9), (13, 10)], ids=str)
def test_base_is_united_with_the_cloud_of_this_call_only(engine, oracle, n):
    s, origin, cell = _fresh(engine, n)
    before = _field(engine, s)
    with pytest.raises(E.Gpmp2miError) as ei:                  # no base yet
        engine.sdf_update_from_points(s, mc.cloud(n, origin, cell, 64, 1), use_base=True)
    assert ei.value.code == 1 and "base" in str(ei.value)
    np.testing.assert_array_equal(_field(engine, s), before)   # a refused call changes nothing
    occ = mc.random_occupancy(n, seed=3)
    engine.sdf_update_from_occupancy(s, occ)
    base_field = mr.field_of(oracle, occ, cell)
    np.testing.assert_array_equal(_field(engine, s), base_field)
    for seed in (11, 12):                                      # two successive clouds: the first one is gone
        pts = mc.cloud(n, origin, cell, 65, seed)
        want, want_stats, _ = mr.update_from_points(oracle, n, origin, cell, pts, base=occ)
        assert engine.sdf_update_from_points(s, pts, use_base=True) == want_stats
        np.testing.assert_array_equal(_field(engine, s), want)
    assert engine.sdf_update_from_points(s, np.zeros((0, len(n))), use_base=True) == dict(kept=0, non_finite=0, self=0, outside=0)
    np.testing.assert_array_equal(_field(engine, s), base_field)
    engine.sdf_update(s, before)                               # a plain update clears the base
    with pytest.raises(E.Gpmp2miError) as ei:
        engine.sdf_update_from_points(s, np.zeros((0, len(n))), use_base=True)
    assert ei.value.code == 1
    np.testing.assert_array_equal(_field(engine, s), before)


# ---------------------------------------------------------------------------------------------- 3. self filter
@pytest.mark.parametrize("margin", [0.0, 0.05])
@pytest.mark.parametrize("setup", ["wam", "point2d"])
def test_self_filter_drops_the_points_inside_the_body_spheres(engine, oracle, setup, margin):
    g = mc.self_setup(setup)
    centers, radii, lo, hi = mc.self_setup_cpu(oracle, setup)
    pts = mc.self_cloud(centers, radii, lo, hi, seed=7)
    # a point within 1e-9 of a boundary could get another verdict from the device's centres (last-bit different)
    band = mr.boundary_band(pts, centers, radii, margin)
    assert band.sum() <= 0.01 * len(pts)
    pts = pts[~band]
    r, s = engine.robot(g["model"]), engine.sdf(g["origin"], g["cell"], g["data"])
    np.testing.assert_allclose(engine.sphere_centers(r, g["conf"])[0][0], centers, atol=1e-12)
    want, want_stats, _ = mr.update_from_points(oracle, g["n"], g["origin"], g["cell"], pts, None, centers, radii, margin)
    stats = engine.sdf_update_from_points(s, pts, use_base=False, robot=r, conf=g["conf"], margin=margin)
    print(setup, margin, stats)
    assert stats == want_stats and stats["self"] > 0 and stats["kept"] > 0
    np.testing.assert_array_equal(_field(engine, s), want)
    # without the filter the same cloud keeps those points
    assert engine.sdf_update_from_points(s, pts, use_base=False)["self"] == 0


# ---------------------------------------------------------------------------------------------- 4. the packed cells
@pytest.mark.parametrize("n", [(33, 20, 9), (13, 10)], ids=str)
def test_packed_cells_follow_an_update(engine, n):
    s, origin, cell = _fresh(engine, n)
    rng = np.random.default_rng(8)
    o, nn = np.asarray(origin), np.asarray(n)
    q = rng.uniform(o - 2 * cell, o + (nn + 1) * cell, size=(500, len(n)))       # some out of range
    data = rng.normal(size=mr.grid_shape(n))
    occ = mc.random_occupancy(n, seed=9)
    for update, make in ((lambda: engine.sdf_update(s, data), lambda: engine.sdf(origin, cell, data)),
                         (lambda: engine.sdf_update_from_occupancy(s, occ), lambda: engine.sdf_from_occupancy(origin, cell, occ))):
        update()
        fresh = make()
        got, want = engine.sdf_query(s, q), engine.sdf_query(fresh, q)
        assert 0 < want[2].sum() < len(q)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(_field(engine, s), _field(engine, fresh))


def test_planner_field_classes_update_the_live_handle_and_keep_data_in_step(oracle):
    from gpmp2_amd import planner as P
    n, cell = (10, 8, 6), 0.1
    f3 = P.SignedDistanceField([0.0, 0.0, 0.0], cell, 8, 10, 6)
    for z in range(6):
        f3.initFieldData(z, np.full((8, 10), 0.5))
    f2 = P.PlanarSDF([0.0, 0.0], cell, np.full((8, 10), 0.5))
    for f, dim in ((f3, 3), (f2, 2)):
        h, nn = f.handle(), n[:dim]
        q = [0.5, 0.4, 0.3][:dim]
        assert f.getSignedDistance(q) == 0.5
        occ = mc.random_occupancy(nn, seed=4, p=0.1)
        f.updateFromOccupancy(occ)
        np.testing.assert_array_equal(f.raw_data(), mr.field_of(oracle, occ, cell))
        pts = np.array([[0.5 + dx, 0.4 + dy, 0.3 + dz][:dim] for dx in (-cell, 0, cell) for dy in (-cell, 0, cell) for dz in (-cell, 0, cell)])
        stats = f.updateFromPoints(pts, use_base=True)
        want, want_stats, _ = mr.update_from_points(oracle, nn, [0.0] * dim, cell, pts, base=occ)
        assert stats == want_stats and f.handle() is h                 # the same handle: planners on it see the change
        np.testing.assert_array_equal(f.raw_data(), want)
        assert f.getSignedDistance(q) < 0.0


# ---------------------------------------------------------------------------------------------- 5. plans see it
def _wam_maps(oracle):
    """the 40^3 desk scene as an occupancy grid (map A) and a cloud that adds a box at the hand's place half-way along the
    straight line in configuration space (map B = A united with the box)"""
    p = problems.wam_restarts(B=3, total_step=10, obs_check_inter=2, sdf="40")
    occ_a = (np.asarray(p.sdf_data) < 0.0).astype(np.float64)
    mid = 0.5 * (problems.WAM_START + problems.WAM_END)
    hand = oracle.sphere_centers(oracle.robot(p.model), mid)[0][0][-1]
    k = np.arange(-2, 3) * p.sdf_cell
    box = np.array([[hand[0] + dx, hand[1] + dy, hand[2] + dz] for dz in k for dy in k for dx in k])
    return p, occ_a, box


def _solve(engine, r, s, p):
    pl = engine.plan(r, s, p.setting, p.B)
    out = _resolve(pl, p)
    pl.close()
    return out


def _resolve(pl, p):
    pl.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
    pl.optimize()
    res = pl.result()
    return dict(iters=res["iters"], status=res["status"], final_error=res["final_error"], traj=res["traj"], score=pl.score(2))


def _same(a, b):
    for k in ("iters", "status", "final_error", "traj"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for k in a["score"]:
        np.testing.assert_array_equal(a["score"][k], b["score"][k], err_msg="score " + k)


@pytest.fixture(scope="module")
def wam_maps(oracle):
    return _wam_maps(oracle)


def _opt(p, opt):
    q = problems.wam_restarts(B=3, total_step=10, obs_check_inter=2, opt=opt, sdf="40")
    q.sdf_data = p.sdf_data
    return q


@pytest.fixture(scope="module")
def gn_on_b(engine, oracle, wam_maps):
    """the GN problem solved by a fresh plan on a fresh handle created from map B's field (cases 5 and 7)"""
    p, occ_a, box = wam_maps
    field_b, _, _ = mr.update_from_points(oracle, (40, 40, 40), p.sdf_origin, p.sdf_cell, box, base=occ_a)
    return _solve(engine, engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, field_b), _opt(p, "GN")), field_b


@pytest.mark.parametrize("opt", ["GN", "LM"])
def test_a_plan_sees_the_updated_map(engine, oracle, wam_maps, gn_on_b, opt):
    p0, occ_a, box = wam_maps
    p = _opt(p0, opt)
    r = engine.robot(p.model)
    s = engine.sdf(p.sdf_origin, p.sdf_cell, np.zeros((40, 40, 40)))
    engine.sdf_update_from_occupancy(s, occ_a)
    pl = engine.plan(r, s, p.setting, p.B)
    on_a = _resolve(pl, p)
    stats = engine.sdf_update_from_points(s, box, use_base=True)
    assert stats["kept"] == len(box)
    on_b = _resolve(pl, p)
    if opt == "GN":
        want, field_b = gn_on_b
        np.testing.assert_array_equal(_field(engine, s), field_b)
    else:
        want = _solve(engine, r, engine.sdf(p.sdf_origin, p.sdf_cell, _field(engine, s)), p)
    _same(on_b, want)
    assert any(not np.array_equal(on_a["traj"][b], on_b["traj"][b]) for b in range(p.B))
    engine.sdf_update_from_points(s, np.zeros((0, 3)), use_base=True)          # back to map A
    _same(_resolve(pl, p), on_a)
    pl.close()


# ---------------------------------------------------------------------------------------------- 6. _dev forms
_DEV = r"""
import numpy as np
import torch                      # torch's HIP runtime first, as bench.py does
torch.cuda.init()
import sys
sys.path.insert(0, "tests")
import map_cases as mc
from gpmp2_amd import engine as E
eng = E.Engine()
g = mc.self_setup("wam")
n, origin, cell = g["n"], g["origin"], g["cell"]
r = eng.robot(g["model"])
host, dev_ = eng.sdf(origin, cell, g["data"]), eng.sdf(origin, cell, g["data"])
occ = mc.random_occupancy(n, seed=21, p=0.01)
rng = np.random.default_rng(22)
lo = np.asarray(origin) - 1.5 * cell
clouds = [np.concatenate([mc.cloud(n, origin, cell, 1000, seed), rng.normal(size=(600, 3)) * 0.4]) for seed in (31, 32)]
margin = 0.03
bits = lambda a: np.ascontiguousarray(a).view(np.int64)
dev = torch.device("cuda:0")
traj = torch.zeros(11, 14, dtype=torch.float64, device=dev)
traj[3, :7] = torch.from_numpy(g["conf"]).to(dev)
conf_ptr = traj.data_ptr() + 3 * 14 * 8        # the configuration of support state 3, inside the trajectory tensor
t_occ = torch.from_numpy(occ).to(dev)
t_pts = [torch.from_numpy(c).to(dev) for c in clouds]
t_stats = [torch.full((4,), -7, dtype=torch.int32, device=dev) for _ in clouds]
t_field = torch.from_numpy(g["data"] * 0.5).to(dev)
eng.sdf_reserve_update(dev_)
torch.cuda.synchronize()
st = torch.cuda.Stream(device=dev)
# occupancy, then two clouds in a row on the stream: no host synchronisation in between
eng.sdf_update_from_occupancy_dev(dev_, t_occ, stream=st.cuda_stream)
for p, s in zip(t_pts, t_stats):
    eng.sdf_update_from_points_dev(dev_, p.shape[0], p, True, r, conf_ptr, margin, s, stream=st.cuda_stream)
st.synchronize()
eng.sdf_update_from_occupancy(host, occ)
want = [eng.sdf_update_from_points(host, c, True, r, g["conf"], margin) for c in clouds]
for s, w in zip(t_stats, want):
    assert s.cpu().numpy().tolist() == [w["kept"], w["non_finite"], w["self"], w["outside"]], (s, w)
    assert w["self"] > 0 and w["kept"] > 0
assert np.array_equal(bits(eng.sdf_field(dev_)["data"]), bits(eng.sdf_field(host)["data"]))
q = rng.uniform(lo, lo + (np.asarray(n) + 2) * cell, size=(300, 3))
for a, b in zip(eng.sdf_query(dev_, q), eng.sdf_query(host, q)):
    assert np.array_equal(a, b)
# stats may be None, and no robot
eng.sdf_update_from_points_dev(dev_, 1600, t_pts[0], False, stream=st.cuda_stream)
st.synchronize()
eng.sdf_update_from_points(host, clouds[0], False)
assert np.array_equal(bits(eng.sdf_field(dev_)["data"]), bits(eng.sdf_field(host)["data"]))
# a plain field from a device buffer
eng.sdf_update_dev(dev_, t_field, stream=st.cuda_stream)
st.synchronize()
eng.sdf_update(host, g["data"] * 0.5)
assert np.array_equal(bits(eng.sdf_field(dev_)["data"]), bits(eng.sdf_field(host)["data"]))
for a, b in zip(eng.sdf_query(dev_, q), eng.sdf_query(host, q)):
    assert np.array_equal(a, b)
try:
    eng.sdf_update_from_points_dev(dev_, 1600, t_pts[0], True, stream=st.cuda_stream)   # the plain update cleared the base
    raise SystemExit("use_base without a base was accepted")
except E.Gpmp2miError as e:
    assert e.code == 1
print("MAP DEV OK")
"""


def test_dev_forms_equal_the_host_calls_bit_for_bit():
    """the `_dev` updates from torch tensors on a torch stream, twice in a row after sdf_reserve_update; in a fresh process
    that starts torch's HIP runtime before the library, as bench.py does"""
    assert importlib.util.find_spec("torch") is not None    # not imported here: this process keeps the library's runtime
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + [x for x in [os.environ.get("PYTHONPATH")] if x]))
    r = subprocess.run([sys.executable, "-c", _DEV], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0 and "MAP DEV OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------------------------------------- 7. multi plan
def test_multi_plan_refreshes_its_copies_of_the_field(engine, wam_maps, gn_on_b):
    p0, occ_a, box = wam_maps
    p = _opt(p0, "GN")
    start = engine.replica_counts()
    r = engine.robot(p.model)
    s = engine.sdf(p.sdf_origin, p.sdf_cell, np.zeros((40, 40, 40)))
    engine.sdf_update_from_occupancy(s, occ_a)
    mp = engine.multi_plan(r, s, p.setting, p.B, [0, 0], replicate_all=True)
    assert engine.replica_counts() == (start[0] + 1, start[1] + 1)

    def run():
        mp.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
        mp.optimize()
        return mp.result()

    on_a = run()
    engine.sdf_update_from_points(s, box, use_base=True)
    stale = run()                                                  # an update touches the caller's handle only
    np.testing.assert_array_equal(stale["traj"], on_a["traj"])
    mp.refresh_field()
    on_b, want = run(), gn_on_b[0]
    for k in ("iters", "status", "final_error", "traj"):
        np.testing.assert_array_equal(on_b[k], want[k], err_msg=k)
    assert not np.array_equal(on_b["traj"], on_a["traj"])
    mp.close()
    assert engine.replica_counts() == start
