"""Carried object (include/gpmp2mi.h "carried object") as far as it can be checked without a GPU: the numpy reference of
tests/carried_reference.py against the augmented robot on the CPU oracle and against central differences, and the
input conditions of tests/test_gpu_carried.py, asserted here on the reference alone."""
import copy

import numpy as np
import pytest

import carried_reference as cr
import score_reference as ref


def _case(oracle, name):
    p, traj = cr.plan_case(name)
    return p, traj, oracle.robot(p.model), cr.field_of(oracle, p)


@pytest.mark.parametrize("name", cr.PLAN_CASES)
def test_rows_equal_the_augmented_robots_obstacle_rows(oracle, name):
    """the two references agree: sphere centres through forward_kinematics and the link's body Jacobian, against the
    same spheres appended as body spheres (oracle.obstacle_factor), 1e-9"""
    p, traj, ro, field = _case(oracle, name)
    D, S = p.setting.dof, p.model.nr_body_spheres()
    link0, eps = cr.PLAN_SETS[name]
    conf = np.ascontiguousarray(traj[:, :, :D]).reshape(-1, D)
    for link in (cr.link_of(p.model, link0), cr.SECOND_LINK[name]):
        radius, centers = cr.spheres(65, 105)
        err, H, inr, _ = cr.hinge_rows(oracle, ro, field, conf, link, radius, centers, eps)
        e2, H2 = oracle.obstacle_factor(oracle.robot(cr.augmented(p.model, link, radius, centers)), field.handle, eps, conf)
        scale = max(np.abs(H2[:, S:]).max(), 1.0)
        print(f"{name} link {link}: {int((err > 0).sum())} of {err.size} rows active, {int((~inr).sum())} outside the field; "
              f"max |d err| {np.abs(err - e2[:, S:]).max():.2e}, max |d H| {np.abs(H - H2[:, S:]).max():.2e}")
        assert np.abs(err - e2[:, S:]).max() <= 1e-9 * max(np.abs(e2).max(), 1.0)
        assert np.abs(H - H2[:, S:]).max() <= 1e-9 * scale
        assert (err[~inr] == 0).all() and (H[~inr] == 0).all()


@pytest.mark.parametrize("name", ["arm3", "wam", "config5", "mobile_wam"])
def test_reference_jacobian_agrees_with_central_differences(oracle, name):
    """h = 1e-6, tolerance 1e-6, on rows that stay active at both probes.  The mobile kinds are probed through the
    oracle's retraction: their Jacobian is the one of the Pose2 chart."""
    p, traj, ro, field = _case(oracle, name)
    D = p.setting.dof
    link0, eps = cr.PLAN_SETS[name]
    link = cr.link_of(p.model, link0)
    radius, centers = cr.spheres(65, 105)
    conf = np.ascontiguousarray(traj[:, :, :D]).reshape(-1, D)
    err, H, _, _ = cr.hinge_rows(oracle, ro, field, conf, link, radius, centers, eps)
    h, worst, rows = 1e-6, 0.0, 0
    for k in range(D):
        probes = []
        for sgn in (+1.0, -1.0):
            d = np.zeros((conf.shape[0], 2 * D))
            d[:, k] = sgn * h
            x = oracle.retract(ro, np.concatenate([conf, np.zeros_like(conf)], axis=1), d)[:, :D]
            probes.append(cr.hinge_rows(oracle, ro, field, x, link, radius, centers, eps)[0])
        both = (probes[0] > 0) & (probes[1] > 0) & (err > 0)
        num = (probes[0] - probes[1]) / (2 * h)
        rows += int(both.sum())
        worst = max(worst, float(np.abs(num - H[..., k])[both].max()))
    print(f"{name}: {rows} active (row, coordinate)s, max |numeric - analytic| {worst:.2e}")
    assert rows > 0 and worst <= 1e-6


@pytest.mark.parametrize("A", [64, 65])
@pytest.mark.parametrize("name", list(cr.FACTOR_CASES))
def test_factor_inputs_take_every_branch(oracle, name, A):
    """the factor cases of the GPU file: an active row, an inactive row in the field and a centre outside the field.
    (A = 1 is the first sphere of the same draw: one sphere cannot take all three.)"""
    p, traj, ro, field = _case(oracle, name)
    D = p.setting.dof
    link0, eps = cr.FACTOR_CASES[name]
    radius, centers = cr.spheres(A, 40 + A)
    conf = np.ascontiguousarray(traj[:, :, :D]).reshape(-1, D)
    err, _, inr, _ = cr.hinge_rows(oracle, ro, field, conf, cr.link_of(p.model, link0), radius, centers, eps)
    print(f"{name} A={A}: {int((err > 0).sum())} of {err.size} active, {int((~inr).sum())} outside")
    assert (err > 0).any() and ((err == 0) & inr).any() and (~inr).any()


def test_plan_inputs_take_every_branch(oracle):
    for name in cr.PLAN_CASES:
        p, traj, ro, field = _case(oracle, name)
        D, N = p.setting.dof, p.setting.total_step
        link0, eps = cr.PLAN_SETS[name]
        link = cr.link_of(p.model, link0)
        conf = np.ascontiguousarray(traj[:, 1:N, :D]).reshape(-1, D)
        radius, centers = cr.spheres(65, 105)
        err, _, inr, _ = cr.hinge_rows(oracle, ro, field, conf, link, radius, centers, eps)
        assert (err > 0).any() and ((err == 0) & inr).any() and (~inr).any(), name
        radius, centers = cr.middle_inactive_set(oracle, ro, field, p, traj, link, eps, (1, N - 1))
        err, _, inr, _ = cr.hinge_rows(oracle, ro, field, conf, link, radius, centers, eps)
        assert (err[:, 64:128] == 0).all() and (~inr[:, 64:128]).all(), name          # the middle chunk is skipped
        assert (err[:, :64] > 0).any() and (err[:, 128:] > 0).any(), name             # the outer ones are not


def test_check_inputs_take_every_branch_and_decide_worst(oracle):
    """every check case has an active pair, an inactive one and a centre outside the field; at most 10 % of the check
    rows have a runner-up within 1e-6 of the minimum"""
    close = rows = 0
    for name in cr.CHECK_NAMES:
        p, traj, ro, field = _case(oracle, name)
        link0, _ = cr.PLAN_SETS[name]
        radius, centers = cr.spheres(65, 105)
        for J in [j for n, j in cr.CHECK_CASES if n == name]:
            exp = cr.oracle_carried_score(oracle, p.model, ro, field, cr.link_of(p.model, link0), radius, centers,
                                          ref.delta_t(p.setting), J, traj)
            clr = exp["clearance"]
            assert (clr < 0).any() and (np.isfinite(clr) & (clr > 0)).any() and (exp["out_of_range"] > 0).all(), (name, J)
            assert (exp["carried_dense_cost"] > 0).any(), (name, J)
            close += cr.close_rows(exp)
            rows += traj.shape[0]
    print(f"{close} of {rows} rows have a runner-up within 1e-6")
    assert close <= 0.1 * rows


def test_the_augmented_robot_is_the_whole_plan_and_the_object_matters(oracle):
    """I = 0, the setting's epsilon and sigma, all states: oracle.linearize of the augmented robot is the reference's
    linearization, oracle.batch_optimize of it is the reference loop, and the loop with and without the object differ
    by more than 1e-2"""
    p, c = cr.scenario()
    ro, field = oracle.robot(p.model), cr.field_of(oracle, p)
    q = cr.augmented_problem(p, c)
    ra = oracle.robot(q.model)
    a = cr.linearize(oracle, ro, field, p, p.init, c)
    b = oracle.linearize(ra, field.handle, p.setting, *cr._args(p), p.init)
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-9 * np.abs(y).max())
    np.testing.assert_allclose(a[3], b[3], rtol=1e-9)
    k = copy.deepcopy(p)
    k.setting.fixed_iterations = cr.ITERS
    with_ = cr.gauss_newton(oracle, ro, field, k, c, cr.ITERS)
    plain = cr.gauss_newton(oracle, ro, field, k, None, cr.ITERS)
    aug = oracle.batch_optimize(ra, field.handle, k.setting, *cr._args(k), k.init)
    print(f"GN x{cr.ITERS}: |reference - augmented batch_optimize| {np.abs(with_ - aug['traj']).max():.2e}; the object moves "
          f"the reference by {np.abs(with_ - plain).max():.2e}")
    assert np.abs(with_ - aug["traj"]).max() <= 1e-6
    assert np.abs(with_ - plain).max() > 1e-2
