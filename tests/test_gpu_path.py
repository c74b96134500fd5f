"""Workspace path on the device (include/gpmp2mi.h "workspace path") against the numpy reference on the CPU oracle
(tests/path_reference.py): the fused factor, the plan's normal equations and graph error with the factor, whole solves
(Gauss-Newton, LM, Dogleg, a queue run), the check of the executed trajectory with its selection, the argument and state
errors that need a live plan, and that plans without capacity are left alone.

Tolerances are the project's own (tests/test_gpu_moving.py): rows rtol 1e-9, normal equations atol 1e-9 max|ref|, errors
rtol 1e-9, final error rtol 1e-8, solved trajectories 1e-6 with identical iterations and status, deviations atol 1e-9,
costs rtol 1e-8."""
import copy
import ctypes as C

import numpy as np
import pytest

import moving_reference as mr
import path_reference as pr
import score_reference as ref
from gpmp2_amd import _capi, scoring
from gpmp2_amd import engine as E
from test_gpu_moving import _DevArray

pytestmark = pytest.mark.gpu
SIX = scoring.PATH_NAMES
_args = pr._args


def _bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    if x.dtype == np.float64:
        x, y = x.view(np.int64), y.view(np.int64)
    return np.array_equal(x, y)


def _same_bits(a, b, what="", names=SIX):
    for k in names:
        assert _bits(a[k], b[k]), (what, k, a[k], b[k])


def _handles(engine, oracle, p):
    return (engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data),
            oracle.robot(p.model), oracle.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data))


def _path_plan(engine, r, s, p, mode, link, B=None):
    q = copy.deepcopy(p)
    q.setting.set_workspace_path(mode, link)
    return q, engine.plan(r, s, q.setting, B or q.B)


# ------------------------------------------------------------------------------------------------------ the factor
@pytest.mark.parametrize("mode", [pr.POSITION, pr.ORIENTATION, pr.POSE])
@pytest.mark.parametrize("name", list(pr.FACTOR_CASES))
def test_factor_matches_the_reference(engine, oracle, name, mode):
    """targets at a known offset from the configuration's own pose; evaluation 0 sits on its target, evaluation 1 is
    1e-5 rad away from it (the Taylor branch of the log map)"""
    p, traj = pr.plan_case(name)
    D, link = p.setting.dof, pr.FACTOR_CASES[name]
    r, ro = engine.robot(p.model), oracle.robot(p.model)
    conf = np.ascontiguousarray(traj[0, :, :D])
    rng = np.random.default_rng(40 + mode)
    own = pr.link_poses(oracle, ro, conf, link)
    des = pr.offset_targets(own, rng)
    # evaluation 0 on its target: the rotation of the device's forward kinematics, and the translation the fused code
    # itself computes (its POSITION residual against the origin), so that t - t_des is an exact zero
    t_own, _ = engine.workspace_path_factor(r, pr.POSITION, link, conf[:1], np.eye(4)[None], jac=False)
    des[0] = engine.forward_kinematics(r, conf[:1])[0][0, link]
    des[0, :3, 3] = t_own[0]
    u = np.array([0.6, -0.48, 0.64])
    des[1] = own[1] @ pr.pose(pr.rot_exp(1e-5 * u), (1e-3, -2e-3, 1e-3))
    err, H = engine.workspace_path_factor(r, mode, link, conf, des)
    e_ref, H_ref = pr.rows(oracle, ro, mode, link, conf, des)
    assert err.shape == (conf.shape[0], pr.nrows(mode)) and np.isfinite(err).all() and np.isfinite(H).all()
    if mode == pr.POSITION:
        assert (err[0] == 0.0).all()
    else:   # R_des^T R is the identity up to the rounding of nine products: a few ulp
        assert np.abs(err[0]).max() <= 1e-15
    assert np.abs(H[0]).max() > 0
    if mode != pr.POSITION:
        np.testing.assert_allclose(np.linalg.norm(e_ref[1, :3]), 1e-5, rtol=1e-6)
    de, dH = np.abs(err - e_ref).max(), np.abs(H - H_ref).max()
    print(f"{name} mode {mode}: max |d err| {de:.2e} of {np.abs(e_ref).max():.2e}, max |d H| {dH:.2e} of "
          f"{np.abs(H_ref).max():.2e}")
    # rows rtol 1e-9; the floor is the rounding of the O(1) coordinates a residual is the difference of
    np.testing.assert_allclose(err[1:], e_ref[1:], rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose(err[0], e_ref[0], rtol=0, atol=1e-14)
    assert dH <= 1e-9 * np.abs(H_ref).max()
    e_only, none = engine.workspace_path_factor(r, mode, link, conf, des, jac=False)
    assert none is None and _bits(e_only, err)


# -------------------------------------------------------------------------------------- linearize and graph error
def _compare_linearize(pl, oracle, ro, so, p, traj, path, label):
    a = pl.linearize(traj)
    b = pr.linearize(oracle, ro, so, p, traj, path)
    worst = [float(np.abs(x - y).max() / np.abs(y).max()) for x, y in zip(a[:3], b[:3])]
    ge = pl.graph_error(traj)
    print(f"{label}: max |d Hd|, |d Ho|, |d g| over max|ref| {worst}, error rel {float(np.abs(a[3] / b[3] - 1.0).max()):.2e}, "
          f"graph_error rel {float(np.abs(ge / b[3] - 1.0).max()):.2e}")
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-9 * np.abs(y).max(), err_msg=label)
    np.testing.assert_allclose(a[3], b[3], rtol=1e-9, err_msg=label)
    np.testing.assert_allclose(ge, b[3], rtol=1e-9, err_msg=label)
    return a


PLAN_MODES = {"arm3": pr.POSE, "wam": pr.POSE, "config5": pr.ORIENTATION, "mobile_wam": pr.POSITION, "pr2": pr.POSE}


@pytest.mark.parametrize("name", mr.PLAN_CASES)
def test_plan_linearize_and_graph_error_carry_the_factor(engine, oracle, name):
    """B = 3: narrow (arm3, WAM, config5: Pose2 chart), wide (mobile WAM, dof 10) and dense (PR2, 190 record entries)
    blocks.  No path is oracle.linearize alone; two time-varying paths in a row are both reflected without recreating
    the plan; states with sigma = +inf and every other block keep the bits of the plan without a path."""
    p, traj = pr.plan_case(name)
    N, D, mode, link = p.setting.total_step, p.setting.dof, PLAN_MODES[name], pr.PLAN_LINKS[name]
    r, s, ro, so = _handles(engine, oracle, p)
    q, pl = _path_plan(engine, r, s, p, mode, link)
    pl.set_problem(*_args(q), q.init)
    base = _compare_linearize(pl, oracle, ro, so, p, traj, None, f"{name} no path")
    for seed, gaps in ((51, (2,)), (52, (0, N))):
        des, sg = pr.time_varying_path(oracle, ro, traj[0], link, seed, gaps=gaps)
        path = dict(mode=mode, link=link, des=des, sigma=sg)
        pl.set_workspace_path(des, sg)
        G, gg, e = pr.plan_terms(oracle, ro, traj, path)
        assert (e > 0).all() and np.abs(G).max() > 0
        got = _compare_linearize(pl, oracle, ro, so, p, traj, path, f"{name} path {seed}")
        for x, y in zip(got, pl.linearize(traj)):
            assert _bits(x, y)                                   # the same bits on a second run
        for i in gaps:                                           # sigma = +inf: the record is not touched
            assert _bits(got[0][:, i], base[0][:, i]) and _bits(got[2][:, i], base[2][:, i]), i
        assert _bits(got[1], base[1])                            # the off-diagonal blocks
        assert _bits(got[0][:, :, D:, :], base[0][:, :, D:, :]) and _bits(got[2][:, :, D:], base[2][:, :, D:])
        # the factor's own share against the reference terms, free of the 1e8 priors that set the scale above
        # (tests/test_gpu_moving.py): 1e-9 of the terms plus the cancellation of the subtraction
        inner = [i for i in range(1, N) if i not in gaps]
        ulp = 8 * np.finfo(np.float64).eps
        dG = np.abs((got[0] - base[0])[:, inner, :D, :D] - G[:, inner]).max()
        dg = np.abs((got[2] - base[2])[:, inner, :D] - gg[:, inner]).max()
        print(f"{name} path {seed}: the factor's share: |d G| {dG:.2e} of {np.abs(G[:, inner]).max():.2e}, |d g| {dg:.2e} of "
              f"{np.abs(gg[:, inner]).max():.2e}")
        assert dG <= 1e-9 * np.abs(G[:, inner]).max() + ulp * np.abs(base[0][:, inner]).max()
        assert dg <= 1e-9 * np.abs(gg[:, inner]).max() + ulp * np.abs(base[2][:, inner]).max()
    # row 1 of the B = 3 plan equals the same problem alone at B = 1, bit for bit
    one = copy.deepcopy(q)
    for k in ("start_conf", "start_vel", "end_conf", "end_vel", "init"):
        setattr(one, k, np.ascontiguousarray(getattr(q, k)[1:2]))
    pl1 = engine.plan(r, s, one.setting, 1)
    pl1.set_problem(*_args(one), one.init)
    pl1.set_workspace_path(des, sg)
    alone = pl1.linearize(traj[1:2])
    for x, y in zip(got, alone):
        assert _bits(x[1:2], y), "row 1 of B = 3 against B = 1"
    pl1.close()
    pl.set_workspace_path(None)                                  # cleared: the plan without a path
    for x, y in zip(base, pl.linearize(traj)):
        assert _bits(x, y)
    pl.close()


def test_path_beside_a_moving_set_and_a_self_collision_row(engine, oracle):
    p, traj = pr.plan_case("wam")
    N, link = p.setting.total_step, 6
    p.setting.self_collision = np.array([[0, 9, 0.6, 0.05]])
    p.setting.self_collision_states = (1, N - 1)
    p.setting.set_moving_spheres(4, mr.EPSILON, mr.SIGMA)
    r, s, ro, so = _handles(engine, oracle, p)
    q, pl = _path_plan(engine, r, s, p, pr.POSE, link)
    pl.set_problem(*_args(q), q.init)
    radius, centers = mr.spheres_near(oracle, p.model, ro, traj, 3, 33, mr.EPSILON)
    des, sg = pr.time_varying_path(oracle, ro, traj[0], link, 53)
    pl.set_moving_spheres(radius, centers)
    pl.set_workspace_path(des, sg)
    mv = dict(radius=radius, centers=centers, epsilon=mr.EPSILON, sigma=mr.SIGMA, states=(0, N))
    want = list(mr.linearize(oracle, ro, so, p, traj, mv))       # oracle (self collision included) + moving terms
    G, gg, e = pr.plan_terms(oracle, ro, traj, dict(mode=pr.POSE, link=link, des=des, sigma=sg))
    D = p.setting.dof
    want[0][:, :, :D, :D] += G
    want[2][:, :, :D] += gg
    want[3] = want[3] + e
    got = pl.linearize(traj)
    for x, y in zip(got[:3], want[:3]):
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-9 * np.abs(y).max())
    np.testing.assert_allclose(got[3], want[3], rtol=1e-9)
    np.testing.assert_allclose(pl.graph_error(traj), want[3], rtol=1e-9)
    pl.close()


# ------------------------------------------------------------------------------------------------------ the solves
def _agree(res, want, label):
    d = np.abs(res["traj"] - want["traj"]).max()
    print(f"{label}: iters {list(res['iters'])} (reference {list(want['iters'])}), max |traj - reference| {d:.2e}, "
          f"final_error rel {np.abs(res['final_error'] / want['final_error'] - 1).max():.2e}")
    assert list(res["iters"]) == list(want["iters"]) and list(res["status"]) == list(want["status"]), label
    assert d <= 1e-6, label
    np.testing.assert_allclose(res["final_error"], want["final_error"], rtol=1e-8, err_msg=label)


@pytest.mark.parametrize("opt", ["GN", "LM", "DOGLEG"])
def test_constant_orientation_path_solves_like_one_workspace_factor(engine, oracle, opt):
    """(a): a constant ORIENTATION target on all states against the same plan with one existing workspace factor over
    0..N"""
    p, link, sigma = pr.constant_orientation_problem(opt)
    r, s, ro, so = _handles(engine, oracle, p)
    N = p.setting.total_step
    hold = pr.link_poses(oracle, ro, p.start_conf[:1], link)[0]
    q, pl = _path_plan(engine, r, s, p, pr.ORIENTATION, link)
    pl.set_workspace_path(np.repeat(hold[None], N + 1, 0), sigma)
    pl.set_problem(*_args(q), q.init)
    pl.optimize()
    res = pl.result()
    n = copy.deepcopy(p)
    n.setting.add_workspace_prior(pr.ORIENTATION, link, hold, sigma, 0, N)
    pn = engine.plan(r, s, n.setting, n.B)
    pn.set_problem(*_args(n), n.init)
    pn.optimize()
    _agree(res, pn.result(), f"(a) {opt}")
    assert (res["iters"] >= 2).all()
    pl.close()
    pn.close()


@pytest.mark.parametrize("opt", ["GN", "LM", "DOGLEG"])
def test_piecewise_pose_path_solves_like_the_oracle_with_native_factors(engine, oracle, opt):
    """(b): a four-range piecewise-constant POSE path against the oracle's own solve through its workspace list"""
    p, link, sigma = pr.piecewise_problem(opt)
    r, s, ro, so = _handles(engine, oracle, p)
    P4 = pr.piecewise_targets(oracle, ro, p, link)
    q, pl = _path_plan(engine, r, s, p, pr.POSE, link)
    pl.set_workspace_path(pr.piecewise_path(P4, p.setting.total_step), sigma)
    pl.set_problem(*_args(q), q.init)
    pl.optimize()
    want = oracle.batch_optimize(ro, so, pr.native_setting(p, pr.POSE, link, P4, sigma), *_args(p), p.init)
    _agree(pl.result(), want, f"(b) {opt}")
    pl.close()


@pytest.fixture(scope="module")
def line(engine, oracle):
    p, link = pr.line_problem()
    p.setting.fixed_iterations = pr.ITERS
    r, s, ro, so = _handles(engine, oracle, p)
    return dict(p=p, link=link, r=r, s=s, ro=ro, so=so, path=pr.line_path(oracle, ro, p, link))


def test_position_line_solves_like_the_reference_loop_and_binds(engine, oracle, line):
    """(c): a time-varying POSITION line against the numpy loop; the tool stays at least 10 times closer to the line
    than in the same problem solved without the path"""
    w = line
    p, path = w["p"], w["path"]
    q, pl = _path_plan(engine, w["r"], w["s"], p, pr.POSITION, w["link"])
    pl.set_workspace_path(path["des"], path["sigma"])
    pl.set_problem(*_args(q), q.init)
    pl.optimize()
    res = pl.result()
    want = pr.gauss_newton(oracle, w["ro"], w["so"], p, path, pr.ITERS)
    d = np.abs(res["traj"] - want).max()
    assert list(res["iters"]) == [pr.ITERS] * p.B and d <= 1e-6
    np.testing.assert_allclose(res["final_error"], pr.graph_error(oracle, w["ro"], w["so"], p, res["traj"], path), rtol=1e-8)
    with_ = pl.path_score(0)["max_pos_dev"]
    pl.set_workspace_path(None)                                  # the same plan solves the problem without the factor
    pl.set_problem(*_args(q), q.init)
    pl.optimize()
    free = pl.result()["traj"]
    assert np.abs(free - pr.gauss_newton(oracle, w["ro"], w["so"], p, None, pr.ITERS)).max() <= 1e-6
    dt = ref.delta_t(p.setting)
    without = engine.path_score_traj(w["r"], pr.POSITION, w["link"], path["des"], path["sigma"], dt, 0, free)["max_pos_dev"]
    print(f"(c) GN x{pr.ITERS}: max |traj - reference| {d:.2e}; max_pos_dev with the path {with_}, without {without}")
    assert (10.0 * with_ <= without).all()
    pl.close()


def test_queue_run_carries_the_resident_path(engine, oracle, line):
    """M = 2 B = 6 problems through B = 3 slots"""
    w = line
    p6, _ = pr.line_problem(B=6)
    p6.setting.fixed_iterations = pr.ITERS
    q, pl = _path_plan(engine, w["r"], w["s"], p6, pr.POSITION, w["link"], B=3)
    pl.set_workspace_path(w["path"]["des"], w["path"]["sigma"])
    res = pl.optimize_queue(*_args(q), q.init)
    want = pr.gauss_newton(oracle, w["ro"], w["so"], p6, w["path"], pr.ITERS)
    d = np.abs(res["traj"] - want).reshape(6, -1).max(axis=1)
    print(f"queue 6 through 3: max |traj - reference| per problem {d}")
    assert list(res["iters"]) == [pr.ITERS] * 6 and d.max() <= 1e-6
    pl.close()


# ------------------------------------------------------------------------------------------ the check, the selection
def _check_against_reference(dev, exp, label):
    B = len(exp["invalid"])
    dp, dr = np.abs(dev["max_pos_dev"] - exp["max_pos_dev"]).max(), np.abs(dev["max_rot_dev"] - exp["max_rot_dev"]).max()
    print(f"{label}: max |d max_pos_dev| {dp:.2e}, |d max_rot_dev| {dr:.2e}, dense_cost rel "
          f"{np.abs(dev['dense_cost'] / np.where(exp['dense_cost'] == 0, 1, exp['dense_cost']) - 1).max():.2e}, invalid {list(dev['invalid'])}")
    assert dp <= 1e-9 and dr <= 1e-9, label
    assert np.array_equal(dev["invalid"], exp["invalid"]), label
    np.testing.assert_allclose(dev["support_cost"], exp["support_cost"], rtol=1e-8, atol=1e-12, err_msg=label)
    np.testing.assert_allclose(dev["dense_cost"], exp["dense_cost"], rtol=1e-8, atol=1e-12, err_msg=label)
    for col, gap in ((0, exp["gap_pos"]), (1, exp["gap_rot"])):   # a runner-up within 1e-6 may take the place
        for b in range(B):
            if not gap[b] <= 1e-6:
                assert dev["worst"][b, col] == exp["worst"][b, col], (label, b, col, dev["worst"], exp["worst"])


@pytest.fixture(scope="module")
def solved(engine, oracle, line):
    """the line problem with a POSE path (the geodesic between the two tool poses) whose middle states carry no factor;
    rows 0 and 2 are the same problem, so their final errors tie"""
    w = line
    p = copy.deepcopy(w["p"])
    p.init[2] = p.init[0]
    N = p.setting.total_step
    path = dict(w["path"], mode=pr.POSE, sigma=np.where(np.isin(np.arange(N + 1), (4, 5)), np.inf, 0.002))
    q, pl = _path_plan(engine, w["r"], w["s"], p, pr.POSE, w["link"])
    pl.set_workspace_path(path["des"], path["sigma"])
    pl.set_problem(*_args(q), q.init)
    pl.optimize()
    return dict(w, p=p, q=q, pl=pl, res=pl.result(), path=path, dt=ref.delta_t(p.setting))


@pytest.mark.parametrize("J", [0, 4])
def test_plan_form_scores_the_bits_of_the_trajectory_form_and_the_reference(engine, oracle, solved, J):
    w = solved
    pl, path, traj = w["pl"], w["path"], w["res"]["traj"]
    through_plan = pl.path_score(J)
    batch = engine.path_score_traj(w["r"], pr.POSE, w["link"], path["des"], path["sigma"], w["dt"], J, traj)
    _same_bits(through_plan, batch, "Plan.path_score vs Engine.path_score_traj on the fetched result")
    _same_bits(through_plan, pl.path_score(J), "Plan.path_score twice in a row")
    exp = pr.oracle_path_score(oracle, w["p"].model, w["ro"], pr.POSE, w["link"], path["des"], path["sigma"], w["dt"], J, traj)
    _check_against_reference(through_plan, exp, f"through the plan, J={J}")
    # the gap: states 4 and 5 and every sub-step that touches them are not checked; both edges are
    chk = ~np.isnan(exp["pos_dev"][0])
    lo, hi = 3 * (J + 1), 6 * (J + 1)
    assert chk[lo] and chk[hi] and not chk[lo + 1:hi].any() and chk[:lo].all() and chk[hi:].all()
    assert (through_plan["max_pos_dev"] > 0).all() and (through_plan["max_rot_dev"] > 0).all()
    assert (through_plan["dense_cost"] >= through_plan["support_cost"]).all()
    part = pl.path_score(J, out={"max_rot_dev": np.zeros(3)})
    assert _bits(part["max_rot_dev"], through_plan["max_rot_dev"])
    # row 1 alone scores the bits it scores in the batch
    alone = engine.path_score_traj(w["r"], pr.POSE, w["link"], path["des"], path["sigma"], w["dt"], J, traj[1])
    for k in SIX:
        assert _bits(alone[k][0], batch[k][1]), k


@pytest.mark.parametrize("mode", [pr.POSITION, pr.ORIENTATION, pr.POSE])
@pytest.mark.parametrize("name,N,J", [("wam", 21, 2), ("wam", 16, 3), ("config5", 16, 3)])
def test_check_matches_the_reference(engine, oracle, name, N, J, mode):
    """Md = 64 and 65 (one record, two records); a NaN row is counted in invalid and excluded"""
    model = mr.check_models()[name]()
    r, ro = engine.robot(model), oracle.robot(model)
    traj = np.array(mr.check_traj(name, N))
    link = pr.FACTOR_CASES[name]
    des, sg = pr.time_varying_path(oracle, ro, traj[0], link, 60 + mode, gaps=(N // 2,))
    traj[1, 3, 2] = np.nan     # a joint / the heading: support state 3 of row 1 and the sub-steps around it
    with np.errstate(invalid="ignore"):
        dev = engine.path_score_traj(r, mode, link, des, sg, mr.CHECK_DT, J, traj)
        exp = pr.oracle_path_score(oracle, model, ro, mode, link, des, sg, mr.CHECK_DT, J, traj)
    assert exp["invalid"][1] >= 1 and exp["invalid"][0] == 0
    _check_against_reference(dev, exp, f"{name} N={N} J={J} mode {mode}")
    if mode == pr.POSITION:
        assert (dev["max_rot_dev"] == 0).all() and (dev["worst"][:, 1] == -1).all()
    if mode == pr.ORIENTATION:
        assert (dev["max_pos_dev"] == 0).all() and (dev["worst"][:, 0] == -1).all()


def test_select_path_is_the_extended_rule_on_the_host_outputs(engine, oracle, solved):
    w = solved
    pl, res, J = w["pl"], w["res"], 4
    sc, ob = pl.path_score(J), pl.score(J)
    assert _bits(res["final_error"][0], res["final_error"][2])   # the tie
    pos, rot = sc["max_pos_dev"], sc["max_rot_dev"]
    cases = [(np.inf, np.inf, -np.inf, False), (np.inf, np.inf, 0.0, True), (float(np.sort(pos)[1]), np.inf, -np.inf, False),
             (float(pos.min()), float(rot.max()), -np.inf, False), (np.inf, float(np.sort(rot)[0]), -np.inf, False),
             (0.5 * float(pos.min()), np.inf, -np.inf, False)]
    seen = set()
    for ap, ar, req, rir in cases:
        got = pl.select_path(J, ap, ar, required_clearance=req, require_in_range=rir)
        want = scoring.path_rule(res["final_error"], res["status"], ob["min_clearance"], ob["out_of_range"], req, rir,
                                 pos, rot, sc["invalid"], ap, ar)
        print(f"select_path(pos <= {ap:.4g}, rot <= {ar:.4g}, clearance >= {req}): {got['best']} of {got['n_eligible']}, rule {want}")
        assert (got["best"], got["n_eligible"]) == want, (ap, ar, req, rir)
        seen.add(want)
        if want[0] >= 0:
            assert _bits(got["traj_best"], res["traj"][want[0]])
        else:
            assert got["traj_best"] is None and got["dense_best"] is None
    assert (-1, 0) in seen and any(n == 3 for _, n in seen)
    # the tie between rows 0 and 2 goes to the lower row whenever both are eligible and best
    every = pl.select_path(J, required_clearance=-np.inf)
    if every["best"] in (0, 2):
        assert every["best"] == 0
    # no path and +inf allowances: gpmp2mi_plan_select, bit for bit
    pl.set_workspace_path(None)
    for req, rir in ((-np.inf, False), (0.0, True)):
        a, b = pl.select_path(J, required_clearance=req, require_in_range=rir), pl.select(J, req, rir)
        assert (a["best"], a["n_eligible"]) == (b["best"], b["n_eligible"])
        if b["best"] >= 0:
            assert _bits(a["traj_best"], b["traj_best"]) and _bits(a["dense_best"], b["dense_best"])
    empty = pl.path_score(J)
    assert (empty["max_pos_dev"] == 0).all() and (empty["worst"] == -1).all() and (empty["dense_cost"] == 0).all()
    pl.set_workspace_path(w["path"]["des"], w["path"]["sigma"])


def test_the_dev_forms_take_and_write_device_buffers(engine, solved):
    w = solved
    pl, path, J, B = w["pl"], w["path"], 2, 3
    N, D = w["q"].setting.total_step, w["q"].setting.dof
    Md = scoring.checked_states(N, J)
    traj = w["res"]["traj"]
    host, host_lin = pl.path_score(J), pl.linearize(traj)
    want = pl.select_path(J, required_clearance=-np.inf)
    des, sg = _DevArray(engine, (N + 1, 4, 4), np.float64, data=path["des"]), _DevArray(engine, (N + 1,), np.float64, data=path["sigma"])
    pl.set_workspace_path(None)
    pl.set_workspace_path_dev(des.ptr, sg.ptr)
    for x, y in zip(host_lin, pl.linearize(traj)):               # the list of constrained states built on the device
        assert _bits(x, y)
    FILL = 0x7B
    best, n = _DevArray(engine, (1,), np.int32, FILL), _DevArray(engine, (1,), np.int32, FILL)
    tb, db = _DevArray(engine, (N + 1, 2 * D), np.float64, FILL), _DevArray(engine, (Md, 2 * D), np.float64, FILL)
    mp, inv, worst = (_DevArray(engine, (B,), np.float64, FILL), _DevArray(engine, (B,), np.int32, FILL),
                      _DevArray(engine, (B, 2), np.int32, FILL))
    untouched = tb.read()
    pl.select_path_dev(J, 0.0, 0.0, required_clearance=-np.inf, best=best.ptr, n_eligible=n.ptr, traj_best=tb.ptr, dense_best=db.ptr)
    pl.path_score_dev(J, max_pos_dev=mp.ptr, invalid=inv.ptr, worst=worst.ptr)
    _same_bits(pl.path_score(J), host, "the path given through device buffers")      # waits for the null stream
    assert (int(best.read()[0]), int(n.read()[0])) == (-1, 0) and _bits(tb.read(), untouched)
    assert _bits(mp.read(), host["max_pos_dev"]) and np.array_equal(inv.read(), host["invalid"])
    assert np.array_equal(worst.read(), host["worst"])
    pl.select_path_dev(J, required_clearance=-np.inf, best=best.ptr, n_eligible=n.ptr, traj_best=tb.ptr, dense_best=db.ptr)
    pl.path_score(J)
    assert (int(best.read()[0]), int(n.read()[0])) == (want["best"], want["n_eligible"]) and want["best"] >= 0
    assert _bits(tb.read(), want["traj_best"]) and _bits(db.read(), want["dense_best"])
    for b in (des, sg, best, n, tb, db, mp, inv, worst):
        b.free()
    pl.set_workspace_path(path["des"], path["sigma"])


# ------------------------------------------------------------------------------------------------ errors and state
def test_errors_that_need_a_live_plan(engine, oracle, line):
    w = line
    p, path, link, lib = w["p"], w["path"], w["link"], engine.lib
    N = p.setting.total_step
    q, pl = _path_plan(engine, w["r"], w["s"], p, pr.POSE, link)
    pl.set_workspace_path(path["des"], path["sigma"])
    for call in (lambda: pl.path_score(1), lambda: pl.select_path(1)):       # nothing to score yet
        with pytest.raises(E.Gpmp2miError) as ei:
            call()
        assert ei.value.code == 1 and "not been optimized" in str(ei.value)
    pl.set_problem(*_args(q), q.init)
    before = pl.linearize(q.init)

    def edited(fn, sigma=None):
        d, s = path["des"].copy(), (path["sigma"].copy() if sigma is None else sigma)
        fn(d, s)
        return d, s

    def nan_entry(d, s): d[3, 1, 2] = np.nan
    def inf_entry(d, s): d[0, 0, 3] = np.inf
    def skewed(d, s): d[5, :3, :3] = d[5, :3, :3] @ np.diag([1.0, 1.0, 1.0 + 1e-5])
    def zero_sigma(d, s): s[2] = 0.0
    def neg_sigma(d, s): s[N] = -0.1
    def nan_sigma(d, s): s[0] = np.nan
    def half_turn(d, s): d[7, :3, :3] = d[6, :3, :3] @ pr.rot_exp([0.0, 0.0, np.pi - 5e-4])
    for fn in (nan_entry, inf_entry, skewed, zero_sigma, neg_sigma, nan_sigma, half_turn):
        with pytest.raises(E.Gpmp2miError) as ei:
            pl.set_workspace_path(*edited(fn))
        assert ei.value.code == 1, fn.__name__
    assert lib.gpmp2mi_plan_set_workspace_path(pl.h.ptr, E.dptr(path["des"]), None) == 1
    for x, y in zip(before, pl.linearize(q.init)):               # a refused call changes nothing
        assert _bits(x, y)
    # what is allowed: the half turn across an unconstrained state, a rotation within 1e-6 of orthonormal, +inf sigma
    def across_gap(d, s):
        half_turn(d, s)
        s[7] = np.inf
    def nearly(d, s): d[5, :3, :3] = d[5, :3, :3] @ np.diag([1.0, 1.0, 1.0 + 1e-7])
    for fn in (across_gap, nearly):
        pl.set_workspace_path(*edited(fn))
    pl.set_workspace_path(path["des"], np.full(N + 1, np.inf))   # no constrained state: nothing is launched
    none = pl.linearize(q.init)
    pl.set_workspace_path(None)
    for x, y in zip(none, pl.linearize(q.init)):
        assert _bits(x, y)
    pl.optimize()
    assert lib.gpmp2mi_plan_path_score(pl.h.ptr, -1, None, None, None, None, None, None) == 1
    assert lib.gpmp2mi_plan_path_score(pl.h.ptr, 1, None, None, None, None, None, None) == 0      # every output may be NULL
    pl.close()
    # a POSITION plan takes the half turn: no rotation is interpolated there
    q0, plp = _path_plan(engine, w["r"], w["s"], p, pr.POSITION, link)
    plp.set_workspace_path(*edited(half_turn))
    plp.close()
    # a plan created without capacity refuses the setter and the plan forms
    pl0 = engine.plan(w["r"], w["s"], p.setting, p.B)
    pl0.set_problem(*_args(p), p.init)
    pl0.optimize()
    for call in (lambda: pl0.set_workspace_path(path["des"], path["sigma"]), lambda: pl0.set_workspace_path(None),
                 lambda: pl0.path_score(1), lambda: pl0.select_path(1)):
        with pytest.raises(E.Gpmp2miError) as ei:
            call()
        assert ei.value.code == 1 and "without workspace_path" in str(ei.value)
    pl0.close()
    # creation: the fields are validated before anything is allocated
    for flag, mode, lk in ((1, 3, link), (1, -1, link), (1, pr.POSE, 7), (1, pr.POSE, -1), (2, pr.POSE, link)):
        st, o, keep = _capi.make_settings(p.setting)
        o.workspace_path, o.workspace_path_mode, o.workspace_path_link = flag, mode, lk
        out = C.c_void_p()
        assert lib.gpmp2mi_plan_create(w["r"].ptr, w["s"].ptr, C.byref(st), C.byref(o), p.B, C.byref(out)) == 1, (flag, mode, lk)
        assert out.value is None


@pytest.mark.parametrize("opt", ["GN", "LM"])
def test_plans_without_a_path_are_left_alone(engine, opt):
    """a plan created without workspace_path against one with capacity and a cleared path (and one whose mode / link
    fields hold junk that is not read without the flag): the same bits from linearize"""
    from gpmp2_amd import problems
    p = problems.wam_restarts(B=3, total_step=10, obs_check_inter=2, sdf="40", opt=opt)
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    plain = engine.plan(r, s, p.setting, p.B)
    q, cap = _path_plan(engine, r, s, p, pr.POSE, 6)
    cap.set_workspace_path(np.tile(np.eye(4), (11, 1, 1)), 0.1)
    cap.set_workspace_path(None)
    junk = copy.deepcopy(p)
    junk.setting.workspace_path = None
    pj = E.Plan.__new__(E.Plan)
    pj.eng, pj.robot, pj.sdf, pj.setting, pj.B = engine, r, s, p.setting, p.B
    st, o, keep = _capi.make_settings(p.setting)
    o.workspace_path, o.workspace_path_mode, o.workspace_path_link = 0, 9, -4
    pj._keep = (st, o, keep)
    out = C.c_void_p()
    engine._ck(engine.lib.gpmp2mi_plan_create(r.ptr, s.ptr, C.byref(st), C.byref(o), p.B, C.byref(out)))
    pj.h = E._Handle(out, engine.lib.gpmp2mi_plan_destroy)
    pj.D, pj.N = p.setting.dof, p.setting.total_step
    results = []
    for pl in (plain, cap, pj):
        pl.set_problem(*_args(p), p.init)
        lin = pl.linearize(p.init)
        pl.optimize()
        results.append((lin, pl.result()))
        pl.close()
    assert (results[0][1]["iters"] >= 1).all()
    for lin, res in results[1:]:
        for x, y in zip(results[0][0], lin):
            assert _bits(x, y)
    # without the flag the whole solve keeps its bits.  A plan with capacity is driven like every plan with extra
    # factors (no early stop: the error is summed from per-block instead of per-chunk shares, another order), so its
    # solve is held to the project's solve tolerances
    for k in ("traj", "final_error", "iters", "status"):
        assert np.array_equal(results[0][1][k], results[2][1][k]), k
    _agree(results[1][1], results[0][1], f"capacity and a cleared path, {opt}")
