"""Workspace path (include/gpmp2mi.h "workspace path") as far as it can be checked without a GPU: the reference of
tests/path_reference.py against the CPU oracle's native workspace factors, its SO(3) maps at their branch edges, and the
inputs of the whole-solve cases of tests/test_gpu_path.py."""
import copy

import numpy as np
import pytest

import path_reference as pr


def _handles(oracle, p):
    return oracle.robot(p.model), oracle.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)


@pytest.mark.parametrize("mode", [pr.POSITION, pr.ORIENTATION, pr.POSE])
@pytest.mark.parametrize("name", ["wam", "config5"])
def test_piecewise_constant_path_equals_four_native_workspace_factors(oracle, name, mode):
    """the reference's normal equations and graph error against oracle.linearize of the same problem with the four
    ranges as native workspace factors, rtol 1e-12"""
    p, traj = pr.plan_case(name)
    ro, so = _handles(oracle, p)
    link, N, sigma = pr.PLAN_LINKS[name], p.setting.total_step, 0.03
    P4 = pr.offset_targets(pr.piecewise_targets(oracle, ro, p, link), np.random.default_rng(4))
    path = dict(mode=mode, link=link, des=pr.piecewise_path(P4, N), sigma=np.full(N + 1, sigma))
    got = pr.linearize(oracle, ro, so, p, traj, path)
    q = copy.deepcopy(p)
    q.setting = pr.native_setting(p, mode, link, P4, sigma)
    want = oracle.linearize(ro, so, q.setting, *pr._args(q), traj)
    plain = oracle.linearize(ro, so, p.setting, *pr._args(p), traj)
    assert np.abs(want[0] - plain[0]).max() > 0 and (want[3] > plain[3]).all()      # the factors are there
    for x, y in zip(got[:3], want[:3]):
        np.testing.assert_allclose(x, y, rtol=1e-12, atol=1e-12 * np.abs(y).max())
    np.testing.assert_allclose(got[3], want[3], rtol=1e-12)
    np.testing.assert_allclose(pr.graph_error(oracle, ro, so, p, traj, path),
                               oracle.graph_error(ro, so, q.setting, *pr._args(q), traj), rtol=1e-12)
    # a state with sigma = +inf adds nothing
    gap = dict(path, sigma=np.where(np.arange(N + 1) == 3, np.inf, sigma))
    G, gg, _ = pr.plan_terms(oracle, ro, traj, gap)
    assert not G[:, 3].any() and not gg[:, 3].any() and G[:, 2].any()


@pytest.mark.parametrize("theta", [0.0, 1e-9, 1.0, np.pi - 2e-3])
def test_exp_and_log_round_trip(theta):
    u = np.array([0.6, -0.48, 0.64])
    w = theta * u
    R = pr.rot_exp(w)
    np.testing.assert_allclose(R.T @ R, np.eye(3), atol=1e-15 + theta * theta * (theta < 1e-6))
    back = pr.rot_log(R)
    # near pi, with t = pi - theta: cos(theta) = -1 + t^2 / 2, so a rounding error eps of the trace is a relative error
    # eps / t^2 of t, and the logarithm's factor theta / (2 sin(theta)) carries it: eps / sin(theta)^2, a few of them
    tol = 1e-15 if theta < 1e-6 else 4 * np.finfo(np.float64).eps / np.sin(theta) ** 2
    np.testing.assert_allclose(back, w, rtol=0, atol=tol * max(theta, 1.0))
    np.testing.assert_allclose(pr.rot_exp(back), R, rtol=0, atol=max(tol, 1e-14))
    xi = pr.pose_log(R, np.array([0.1, 0.2, -0.3]))
    np.testing.assert_allclose(xi[:3], back, rtol=0, atol=0)
    if theta == 0.0:
        assert np.array_equal(R, np.eye(3)) and np.array_equal(xi[3:], [0.1, 0.2, -0.3])


def test_checked_targets_between_support_states():
    A, B = pr.pose(t=(0.0, 0.0, 0.0)), pr.pose(pr.rot_exp([0.0, 0.0, 1.0]), (1.0, 2.0, 4.0))
    des = np.stack([A, B, B])
    T, sg, chk = pr.checked_targets(des, [0.1, 0.3, np.inf], 3, pr.POSE)
    assert T.shape == (9, 4, 4) and list(chk) == [True] * 5 + [False] * 4
    assert np.array_equal(T[0], A) and np.array_equal(T[4], B)
    assert np.array_equal(T[1, :3, 3], [0.25, 0.5, 1.0])
    np.testing.assert_allclose(pr.rot_log(T[2, :3, :3]), [0.0, 0.0, 0.5], atol=1e-15)
    np.testing.assert_allclose(sg[:5], [0.1, 0.15, 0.2, 0.25, 0.3], atol=1e-16)


def _margins(res, setting):
    """how far a converged oracle run stopped from its two thresholds: |last decrease| / abs_error_tol, and the last
    relative decrease over rel_thresh"""
    a = pr.last_decision_margin(res)
    rel = []
    for b in range(len(res["iters"])):
        tr = res["error_trace"][b]
        tr = tr[~np.isnan(tr)]
        rel.append(abs(tr[-2] - tr[-1]) / tr[-2] / setting.rel_thresh)
    return a, np.array(rel)


@pytest.mark.parametrize("opt", ["GN", "LM", "DOGLEG"])
def test_the_convergent_solve_cases_stop_away_from_their_thresholds(oracle, opt):
    """cases (a) and (b) of tests/test_gpu_path.py on the oracle's native workspace factors: no run ends within a
    factor 10 of abs_error_tol at its last decision (nor within 1e-3 of the relative threshold), so identical
    iteration counts are a fair demand of the device"""
    p, link, sigma = pr.constant_orientation_problem(opt)
    ro, so = _handles(oracle, p)
    N = p.setting.total_step
    hold = pr.link_poses(oracle, ro, p.start_conf[:1], link)[0]
    sa = copy.deepcopy(p.setting)
    sa.add_workspace_prior(pr.ORIENTATION, link, hold, sigma, 0, N)
    pb, link, sigma = pr.piecewise_problem(opt)
    sb = pr.native_setting(pb, pr.POSE, link, pr.piecewise_targets(oracle, ro, pb, link), sigma)
    for label, q, s in (("a", p, sa), ("b", pb, sb)):
        res = oracle.batch_optimize(ro, so, s, *pr._args(q), q.init)
        a, rel = _margins(res, s)
        print(f"case ({label}) {opt}: iters {res['iters']}, |last decrease| / abs_error_tol {a}, "
              f"last relative decrease / rel_thresh {rel}")
        assert (res["status"] == 0).all() and (res["iters"] < s.max_iter).all()
        assert ((a > 10.0) | (a < 0.1)).all()
        assert (np.abs(rel - 1.0) > 1e-3).all()


def test_the_line_case_binds(oracle):
    """case (c): the reference loop with the POSITION line keeps the tool at least 10 times closer to the line than
    the loop without it; and the loop without a path is the oracle's own solve"""
    p, link = pr.line_problem()
    ro, so = _handles(oracle, p)
    path = pr.line_path(oracle, ro, p, link)
    with_ = pr.gauss_newton(oracle, ro, so, p, path, pr.ITERS)
    without = pr.gauss_newton(oracle, ro, so, p, None, pr.ITERS)
    a = pr.support_pos_dev(oracle, ro, with_, link, path["des"])
    b = pr.support_pos_dev(oracle, ro, without, link, path["des"])
    print(f"max support |t - line| with the path {a}, without {b}")
    assert (10.0 * a <= b).all()
    q = copy.deepcopy(p)
    q.setting.fixed_iterations = pr.ITERS
    want = oracle.batch_optimize(ro, so, q.setting, *pr._args(q), q.init)
    assert np.array_equal(without.view(np.int64), want["traj"].view(np.int64))
    # the check at J = 0 states the same deviation
    sc = pr.oracle_path_score(oracle, p.model, ro, pr.POSITION, link, path["des"], path["sigma"],
                              p.setting.total_time / p.setting.total_step, 0, with_)
    np.testing.assert_allclose(sc["max_pos_dev"], a, rtol=1e-12)
    assert (sc["max_rot_dev"] == 0).all() and (sc["worst"][:, 1] == -1).all() and (sc["invalid"] == 0).all()
