"""gpmp2mi_ik_solve / _seeded / gpmp2mi_ik_goals (include/gpmp2mi.h "goal configurations") on the device against the
float64 restatement of the rule over the CPU oracle (tests/ik_reference.py), row by row.

Bound of a configuration on the rows both converged on:

    max |conf_gpu - conf_ref| <= min(max(K * d_self, FLOOR), CAP)

d_self is the reference's own move of that row when its seeds move by +-2 ulp (4 trials; tests/test_ik_cpu.py asserts
that no status and no iteration count flips there).  K and FLOOR come from one measured run of every case of this file
(profiles/ik_error.txt, written by scripts/ik_error.py, states the rule and the run): K the next power of two above 4 x
the largest ratio e_gpu / d_self among the rows with d_self >= 1e-15, FLOOR 4 x the largest e_gpu among the rows with
d_self < 1e-15.  CAP is the largest power of ten that both deliberate slips of tests/test_ik_cpu.py exceed
(lambda_factor 4 -> 4.01 moves a row by 7.8e-2, dropping the clamp by 8.7): a condition, not measured on the device.
Status and iters are equal except on at most 2 % of a case's rows."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import gpmp2_amd as g
import ik_reference as ik
import score_reference as sref
from gpmp2_amd import _capi, problems, scoring

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CAP = 1e-2                # both slips of tests/test_ik_cpu.py move a row by more; one of them by less than 1e-1
K = 16.0                  # profiles/ik_error.txt: largest e_gpu / d_self 2.56 (wam_pose) -> next power of two above 4 x that
FLOOR = 4 * 2.220e-15     # profiles/ik_error.txt: largest e_gpu among the rows with d_self < 1e-15 (arm2_position)
SELF_EXACT = 1e-15        # rows whose d_self lies below this set FLOOR
MISMATCH = 0.02           # share of a case's rows whose status / iters may differ


def bound(d_self):
    return np.minimum(np.maximum(K * d_self, FLOOR), CAP)


def _opts(engine, robot, o):
    return engine.ik_opts(robot, o.mode, o.link, (o.down, o.up), pos_tol=o.pos_tol, rot_tol=o.rot_tol, rot_weight=o.rot_weight,
                          max_iter=o.max_iter, lambda_initial=o.lambda_initial, lambda_factor=o.lambda_factor,
                          lambda_lower=o.lambda_lower, lambda_upper=o.lambda_upper)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(a, b, keys=("conf", "residual", "iters", "status"), what=""):
    for k in keys:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


def measure_case(engine, case, ref, d_self, M=None):
    """the device's rows of one case (the first M seed rows of every pose) against the reference: dict(dev, differ [G][M],
    both [G][M], e_gpu [G][M], d_self [G][M])"""
    M = case.M if M is None else M
    r = engine.robot(case.model)
    dev = engine.ik_solve(r, _opts(engine, r, case.opts), case.poses, case.seeds[:, :M])
    st, it = ref["status"][:, :M], ref["iters"][:, :M]
    differ = (dev["status"] != st) | (dev["iters"] != it)
    both = (dev["status"] == ik.CONVERGED) & (st == ik.CONVERGED)
    e = np.where(both, np.abs(dev["conf"] - ref["conf"][:, :M]).max(axis=2), 0.0)
    return dict(dev=dev, differ=differ, both=both, e_gpu=e, d_self=d_self[:, :M])


@pytest.fixture(scope="module")
def ref(oracle):
    return {c.name: (c, r, d, f) for c, r, d, f in ik.reference(oracle)}


def _check_independent(oracle, case, dev):
    """what holds whatever the reference's iteration does"""
    o, ro = case.opts, oracle.robot(case.model)
    for i in range(dev["conf"].shape[0]):
        conf, st = dev["conf"][i], dev["status"][i]
        live = st != ik.INVALID
        assert ((conf[live] >= o.down) & (conf[live] <= o.up)).all()
        e, _ = oracle.workspace_prior_factor(ro, o.mode, o.link, case.poses[i], conf[live])
        res = ik.residual(o, e)
        assert np.abs(res - dev["residual"][i][live]).max() <= 1e-12
        ok = st[live] == ik.CONVERGED
        assert (res[ok, 0] <= o.rot_tol * (1 + 1e-9)).all() and (res[ok, 1] <= o.pos_tol * (1 + 1e-9)).all()
        assert (dev["iters"][i][st == ik.MAX_ITER_REACHED] == o.max_iter).all()
        assert (dev["iters"][i] <= o.max_iter).all()


CASES = [("wam_pose", 1), ("wam_pose", 63), ("wam_pose", 64), ("wam_pose", 65), ("wam_position", 64),
         ("wam_orientation", 64), ("arm3_pose", 64), ("arm2_position", 64), ("planar1_position", 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,M", CASES, ids=[f"{n}-M{m}" for n, m in CASES])
def test_rows_agree_with_the_reference(engine, oracle, ref, name, M):
    case, rf, d_self, flips = ref[name]
    assert not flips.any()                      # the condition under which rows are compared (tests/test_ik_cpu.py)
    m = measure_case(engine, case, rf, d_self, M)
    n_rows, n_diff = m["differ"].size, int(m["differ"].sum())
    over = m["both"] & ~m["differ"] & (m["e_gpu"] > bound(m["d_self"]))
    ratio = np.where(m["both"] & (m["d_self"] >= SELF_EXACT), m["e_gpu"] / np.maximum(m["d_self"], SELF_EXACT), 0.0)
    print(f"{name} M={M}: rows {n_rows}, status/iters differ on {n_diff}, converged on both {int(m['both'].sum())}, "
          f"largest e_gpu {m['e_gpu'].max():.3e}, largest e_gpu / d_self {ratio.max():.1f}")
    assert n_diff <= MISMATCH * n_rows, (name, n_diff, n_rows)
    assert M < 63 or (m["both"].sum(axis=1) >= 8).all()
    assert not over.any(), (name, m["e_gpu"][over], m["d_self"][over])
    _check_independent(oracle, case, m["dev"])


@pytest.mark.gpu
def test_an_invalid_row_leaves_the_other_rows_alone(engine, ref):
    case = ref["wam_pose"][0]
    r = engine.robot(case.model)
    o = _opts(engine, r, case.opts)
    seeds = case.seeds[:, :64].copy()
    clean = engine.ik_solve(r, o, case.poses, seeds)
    seeds[1, 37, 3] = np.nan
    seeds[2, 5, 0] = np.inf
    dirty = engine.ik_solve(r, o, case.poses, seeds)
    assert dirty["status"][1, 37] == ik.INVALID and dirty["status"][2, 5] == ik.INVALID
    assert dirty["iters"][1, 37] == 0 and np.isnan(dirty["conf"][1, 37, 3]) and dirty["conf"][2, 5, 0] == case.opts.up[0]
    keep = np.ones((3, 64), dtype=bool)
    keep[1, 37] = keep[2, 5] = False
    for k in ("conf", "residual", "iters", "status"):
        assert np.array_equal(_bits(dirty[k])[keep], _bits(clean[k])[keep]), k


@pytest.mark.gpu
def test_a_row_is_the_same_alone_anywhere_in_a_batch_and_through_the_seeded_form(engine, ref):
    case = ref["wam_pose"][0]
    r = engine.robot(case.model)
    o = _opts(engine, r, case.opts)
    full = engine.ik_solve(r, o, case.poses, case.seeds)                       # G = 3, M = 65, given seeds
    alone = engine.ik_solve(r, o, case.poses[2:3], case.seeds[2:3, 37:38])      # pose 2, row 37 alone
    one_pose = engine.ik_solve(r, o, case.poses[2:3], case.seeds[2:3, :64])     # row 37 of 64
    for k in ("conf", "residual", "iters", "status"):
        assert np.array_equal(_bits(alone[k])[0, 0], _bits(full[k])[2, 37]), k
        assert np.array_equal(_bits(one_pose[k])[0, 37], _bits(full[k])[2, 37]), k
    # the seeded form draws what rng_reference draws (case.seeds), bit for bit, and `first` shifts the rows
    seeded = engine.ik_solve(r, o, case.poses, M=65, seed=case.seed)
    _same(seeded, full, what="seeded vs given seeds")
    shifted = engine.ik_solve(r, o, case.poses, M=20, seed=case.seed, first=40)
    for k in ("conf", "residual", "iters", "status"):
        assert np.array_equal(_bits(shifted[k]), _bits(full[k])[:, 40:60]), k
    other = engine.ik_solve(r, o, case.poses, M=8, seed=case.seed + 1)
    assert not np.array_equal(other["conf"], full["conf"][:, :8])
    # G = 0 and M = 0 are fine and do nothing
    assert engine.ik_solve(r, o, case.poses, M=0, seed=1)["conf"].shape == (3, 0, 7)


def _two_link(engine, down, up):
    model = g.generateArm("SimpleTwoLinksArm")
    r = engine.robot(model)
    return model, r, engine.ik_opts(r, _capi.WORKSPACE_POSITION, 1, (down, up))


@pytest.mark.gpu
def test_two_link_goals_are_the_two_analytic_branches_in_near_order(engine):
    from test_ik_cpu import _position_pose, _two_link_branches
    x, y = 0.55, 0.35
    want = _two_link_branches(x, y)                       # q2 < 0 first
    model, r, o = _two_link(engine, [-np.pi] * 2, [np.pi] * 2)
    for near, order in ((want[0], (0, 1)), (want[1], (1, 0))):
        gl = engine.ik_goals(r, o, _position_pose(x, y), M=64, seed=7, radius=1e-3, max_goals=4, near=near)
        assert gl["n_goals"][0] == 2 and gl["n_converged"][0] == gl["n_eligible"][0] >= 8
        got = gl["goal_conf"][0, :2]
        assert np.abs(got - want[list(order)]).max() < 1e-3
        assert gl["goal_score"][0, 0] < 1e-3 < gl["goal_score"][0, 1]
        assert (gl["goal_seed"][0, 2:] == -1).all() and np.isnan(gl["goal_conf"][0, 2:]).all()
        assert np.isinf(gl["clearance"]).all() and not gl["out_of_range"].any()        # no field
        for k in range(2):
            assert np.array_equal(gl["conf"][0, gl["goal_seed"][0, k]], got[k])
    # a limit that excludes the q2 > 0 branch leaves one goal
    model, r, o = _two_link(engine, [-np.pi, -np.pi], [np.pi, 0.0])
    gl = engine.ik_goals(r, o, _position_pose(x, y), M=64, seed=7, radius=1e-3, max_goals=4)
    assert gl["n_goals"][0] == 1 and np.abs(gl["goal_conf"][0, 0] - want[0]).max() < 1e-3
    assert (gl["conf"][0, :, 1] <= 0.0).all()
    # out of reach: nothing converges, no goal
    gl = engine.ik_goals(r, o, _position_pose(2.0, 0.0), M=64, seed=7, radius=1e-3, max_goals=4)
    assert gl["n_goals"][0] == 0 and gl["n_converged"][0] == 0 and (gl["goal_seed"] == -1).all() and (gl["mode"] == -1).all()


@pytest.mark.gpu
def test_wam_goals_in_a_field_agree_with_the_oracle_and_the_rule(engine, oracle, ref):
    case = ref["wam_pose"][0]
    p = problems.wam_restarts(B=1, total_step=4, sdf="40")
    r, s = engine.robot(case.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    ro, fld = oracle.robot(case.model), sref.oracle_sdf(oracle, p.sdf_origin, p.sdf_cell, p.sdf_data)
    o = _opts(engine, r, case.opts)
    near, w, radius, req = problems.WAM_END, np.array([1.0, 1.0, 1.0, 1.0, 0.5, 0.5, 0.25]), 0.5, 0.0
    kw = dict(sdf=s, seeds=case.seeds[:, :64], radius=radius, max_goals=6, near=near, weights=w)
    gl = engine.ik_goals(r, o, case.poses, required_clearance=req, **kw)
    solo = engine.ik_solve(r, o, case.poses, case.seeds[:, :64])
    _same(gl, solo, keys=("conf", "status"), what="the goal stage's IK is ik_solve")
    for i in range(case.G):
        clr, oor, near_face = ik.clearance(oracle, case.model, ro, fld, gl["conf"][i])
        np.testing.assert_allclose(gl["clearance"][i], clr, rtol=0, atol=1e-9)
        assert (np.abs(gl["out_of_range"][i].astype(np.int64) - oor) <= near_face).all()
    # the rule on the device's own conf, clearance and out_of_range: with the requirement every answer meets, and with
    # one that some of the converged answers miss (half-way between their smallest and largest clearance: the largest
    # is the base sphere's, which no joint moves), spheres outside the field refused
    cc = gl["clearance"][gl["status"] == ik.CONVERGED]
    mid = 0.5 * float(cc.min() + cc.max())
    for req, rir in ((0.0, False), (mid, True)):
        got = gl if (req, rir) == (0.0, False) else engine.ik_goals(r, o, case.poses, required_clearance=req, require_in_range=rir, **kw)
        _same(got, gl, keys=("conf", "status", "clearance", "out_of_range"), what="the requirement changes no row")
        for i in range(case.G):
            want = ik.goals(got["conf"][i], got["status"][i], got["clearance"][i], got["out_of_range"][i], True, radius, 6,
                            required_clearance=req, require_in_range=rir, near=near, weights=w)
            conv = got["status"][i] == ik.CONVERGED
            decided = np.abs(got["clearance"][i][conv] - req).min() > 1e-9 and want["margin"] > 1e-9
            print(f"required {req:.4f}, pose {i}: converged {want['n_converged']}, eligible {want['n_eligible']}, goals "
                  f"{want['n_goals']}, margin {want['margin']:.2e}")
            assert decided, "a pair or a clearance sits on its threshold: choose another radius"
            assert (got["n_goals"][i], got["n_converged"][i], got["n_eligible"][i]) == (want["n_goals"], want["n_converged"], want["n_eligible"])
            assert np.array_equal(got["mode"][i], want["mode"]) and np.array_equal(got["goal_seed"][i], want["goal_seed"])
            k = min(want["n_goals"], 6)
            lead = want["goal_seed"][:k]
            assert np.array_equal(got["goal_conf"][i, :k], got["conf"][i, lead])
            assert np.array_equal(got["goal_clearance"][i, :k], got["clearance"][i, lead])
            np.testing.assert_allclose(got["goal_score"][i, :k], want["score"][lead], rtol=1e-14, atol=0)
            assert np.isnan(got["goal_conf"][i, k:]).all() and np.isnan(got["goal_score"][i, k:]).all()
        assert got["n_eligible"].sum() >= 1 and (got["n_eligible"] <= got["n_converged"]).all()
        assert req == 0.0 or got["n_eligible"].sum() < got["n_converged"].sum()
    # a required clearance above every clearance: nothing is eligible, nothing is touched beyond the counts
    top = gl["clearance"][np.isfinite(gl["clearance"])].max() + 1.0
    none = engine.ik_goals(r, o, case.poses, required_clearance=top, **kw)
    assert not none["n_eligible"].any() and not none["n_goals"].any() and np.array_equal(none["n_converged"], gl["n_converged"])
    assert (none["goal_seed"] == -1).all() and (none["mode"] == -1).all()
    assert np.isnan(none["goal_conf"]).all() and np.isnan(none["goal_score"]).all() and np.isnan(none["goal_clearance"]).all()
    # without near the score is the row index: the first eligible row leads
    plain = engine.ik_goals(r, o, case.poses, sdf=s, seeds=case.seeds[:, :64], radius=radius, max_goals=6)
    for i in range(case.G):
        el = np.flatnonzero(plain["mode"][i] >= 0)
        assert plain["goal_seed"][i, 0] == (el[0] if el.size else -1)


@pytest.mark.gpu
def test_refusals(engine, ref):
    from test_gpu_robots import _wide_models
    des, lib = np.eye(4), engine.lib
    for model, word in ((problems.mobile_arm_config5().model, b"GPMP2MI_ROBOT_ARM"), (_wide_models()["arm8 (dof 8)"], b"1..7")):
        r = engine.robot(model)
        o = engine.ik_opts(r)
        for call in (lambda: engine.ik_solve(r, o, des, np.zeros((1, 2, r.dof))),
                     lambda: engine.ik_goals(r, o, des, seeds=np.zeros((1, 2, r.dof)))):
            with pytest.raises(Exception) as ei:
                call()
            assert getattr(ei.value, "code", None) == 4 and word in lib.gpmp2mi_last_error(), lib.gpmp2mi_last_error()
    # the argument errors that need the robot's dof (tests/test_ik_abi.py has the others)
    case = ref["arm2_position"][0]
    r = engine.robot(case.model)
    seeds = np.zeros((1, 2, 2))
    for kw in (dict(limits=([1.0, -1.0], [0.0, 1.0])), dict(limits=([np.nan, -1.0], [1.0, 1.0])), dict(link=2), dict(link=-1)):
        with pytest.raises(Exception) as ei:
            engine.ik_solve(r, engine.ik_opts(r, _capi.WORKSPACE_POSITION, **kw), des, seeds)
        assert getattr(ei.value, "code", None) == 1, kw
    with pytest.raises(Exception) as ei:                 # the seeded form needs finite limits
        engine.ik_solve(r, engine.ik_opts(r, _capi.WORKSPACE_POSITION, limits=([-np.inf, -1.0], [1.0, 1.0])), des, M=2, seed=1)
    assert getattr(ei.value, "code", None) == 1
    free = engine.ik_solve(r, engine.ik_opts(r, _capi.WORKSPACE_POSITION), case.poses, case.seeds[:, :8])   # no limits: fine
    assert (free["status"] != ik.INVALID).all()


_DEV = r"""
import numpy as np
import torch                      # torch's HIP runtime first, as bench.py does
torch.cuda.init()
import sys
sys.path.insert(0, "tests")
from gpmp2_amd import engine as E, problems
import gpmp2_amd as g
import ik_reference as ik
eng = E.Engine()
model = g.generateArm("WAMArm")
p = problems.wam_restarts(B=1, total_step=4, sdf="40")
r, s = eng.robot(model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
o = eng.ik_opts(r, limits=(ik.WAM_DOWN, ik.WAM_UP))
G, M, D, K = 2, 70, 7, 5
rng = np.random.default_rng(3)
q = ik.WAM_DOWN + rng.random((G, D)) * (ik.WAM_UP - ik.WAM_DOWN)
poses = eng.forward_kinematics(r, q)[0][:, 6]
seeds = ik.seed_rows(9, G, M, 0, ik.WAM_DOWN, ik.WAM_UP)
host = eng.ik_solve(r, o, poses, seeds)
hostg = eng.ik_goals(r, o, poses, sdf=s, seeds=seeds, radius=0.5, max_goals=K, near=problems.WAM_END)
dev = torch.device("cuda:0")
f = lambda *sh: torch.full(sh, float("nan"), dtype=torch.float64, device=dev)
i = lambda *sh: torch.full(sh, -7, dtype=torch.int32, device=dev)
dp, ds = torch.from_numpy(poses.reshape(G, 16)).to(dev), torch.from_numpy(seeds).to(dev)
out = dict(conf=f(G, M, D), residual=f(G, M, 2), iters=i(G, M), status=i(G, M))
out2 = dict(conf=f(G, M, D), residual=f(G, M, 2), iters=i(G, M), status=i(G, M))
gout = dict(conf=f(G, M, D), status=i(G, M), clearance=f(G, M), out_of_range=i(G, M), mode=i(G, M), n_goals=i(G),
            n_converged=i(G), n_eligible=i(G), goal_conf=f(G, K, D), goal_seed=i(G, K), goal_score=f(G, K), goal_clearance=f(G, K))
torch.cuda.synchronize()
st = torch.cuda.Stream(device=dev)
eng.ik_solve_dev(r, o, G, M, dp, seeds=ds, stream=st.cuda_stream, **out)
eng.ik_solve_dev(r, o, G, M, dp, seed=9, stream=st.cuda_stream, **out2)
eng.ik_goals_dev(r, o, G, M, dp, sdf=s, seeds=ds, radius=0.5, max_goals=K, near=problems.WAM_END, stream=st.cuda_stream, **gout)
with torch.cuda.stream(st):
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got2 = {k: v.cpu().numpy() for k, v in out2.items()}
    gg = {k: v.cpu().numpy() for k, v in gout.items()}
bits = lambda a: np.ascontiguousarray(a).view(np.int64) if a.dtype == np.float64 else a
for k in host:
    assert np.array_equal(bits(got[k]), bits(host[k])), "ik_solve_dev != ik_solve: " + k
    assert np.array_equal(bits(got2[k]), bits(host[k])), "ik_solve_seeded_dev != ik_solve: " + k
for k in hostg:
    assert np.array_equal(bits(gg[k]), bits(hostg[k])), "ik_goals_dev != ik_goals: " + k
assert (hostg["n_converged"] >= 1).all()
eng.ik_solve_dev(r, o, G, M, dp, seeds=ds, status=out["status"], stream=st.cuda_stream)      # any output may be None
eng.ik_goals_dev(r, o, G, M, dp, seeds=ds, n_goals=gout["n_goals"], stream=st.cuda_stream)
st.synchronize()
for bad in (lambda: eng.ik_solve_dev(r, o, G, M, dp, seeds=ds, conf=out["conf"][:, :1]),
            lambda: eng.ik_solve_dev(r, o, G, M, dp[:1], seeds=ds),
            lambda: eng.ik_solve_dev(r, o, G, M, dp, seeds=ds, iters=out["conf"]),
            lambda: eng.ik_goals_dev(r, o, G, M, dp, seeds=ds, max_goals=K, goal_conf=gout["goal_conf"][:, :2]),
            lambda: eng.ik_goals_dev(r, o, G, M, dp, seeds=ds[:, :3])):
    try:
        bad()
        raise SystemExit("a wrong-shape tensor was accepted")
    except ValueError:
        pass
print("IK DEV OK")
"""


@pytest.mark.gpu
def test_dev_forms_equal_the_host_calls_bit_for_bit():
    """the _dev forms into torch tensors on a torch stream; in a fresh process that starts torch's HIP runtime before the
    library, as bench.py does"""
    assert importlib.util.find_spec("torch") is not None    # not imported here: this process keeps the library's runtime
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + [x for x in [os.environ.get("PYTHONPATH")] if x]))
    r = subprocess.run([sys.executable, "-c", _DEV], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0 and "IK DEV OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.gpu
def test_pose_to_goals_to_plan_end_to_end(engine):
    p = problems.wam_restarts(B=4, total_step=5, obs_check_inter=1, opt="GN", sdf="40")
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pose = engine.forward_kinematics(r, problems.WAM_END)[0][0, 6]
    o = engine.ik_opts(r, limits=(ik.WAM_DOWN, ik.WAM_UP))
    gl = engine.ik_goals(r, o, pose, sdf=s, M=64, seed=21, radius=0.5, max_goals=4, near=problems.WAM_END)
    assert gl["n_goals"][0] >= 1
    ends = engine.goal_rows(gl, p.B)
    assert ends.shape == (4, 7)
    N = p.setting.total_step
    init = np.zeros_like(p.init)
    for b in range(p.B):
        init[b] = g.initArmTrajStraightLine(p.start_conf[b], ends[b], N)
    pl = engine.plan(r, s, p.setting, p.B)
    pl.set_problem(p.start_conf, p.start_vel, ends, p.end_vel, init)
    pl.optimize()
    res = pl.result()
    assert res["traj"].shape == (4, N + 1, 14) and res["iters"].shape == (4,) and res["final_error"].shape == (4,)
    assert np.abs(res["traj"][:, -1, :7] - ends).max() <= 10 * p.setting.conf_prior_sigma
    pl.close()
