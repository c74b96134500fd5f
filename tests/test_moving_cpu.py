"""Moving obstacles (include/gpmp2mi.h "moving obstacles") as far as they can be checked without a GPU: the reference of
tests/moving_reference.py against itself and against the CPU oracle, and the inputs of tests/test_gpu_moving.py."""
import copy

import numpy as np
import pytest

import moving_reference as mr
import score_reference as ref


@pytest.fixture(scope="module")
def scen(oracle):
    p, mv = mr.scenario()
    ro, so = oracle.robot(p.model), oracle.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    mv = dict(mv, centers=mr.scenario_centers(oracle, ro, p, mv))
    return p, mv, ro, so


@pytest.mark.parametrize("name", ["arm3", "wam", "config5"])
def test_reference_jacobian_agrees_with_central_differences(oracle, name):
    """h = 1e-6, tolerance 1e-6, on rows that stay active at both probes.  The mobile arm is probed through the
    oracle's retraction: its Jacobian is the one of the Pose2 chart."""
    p, traj = mr.plan_case(name)
    model, D = p.model, p.setting.dof
    ro = oracle.robot(model)
    radius, centers = mr.spheres_near(oracle, model, ro, traj, 4, 3, mr.EPSILON)
    conf = np.ascontiguousarray(traj[0, :, :D])
    cen = centers.transpose(1, 0, 2)
    err, H, _ = mr.hinge_rows(oracle, model, ro, conf, radius, cen, mr.EPSILON)
    h, worst, rows = 1e-6, 0.0, 0
    for k in range(D):
        probes = []
        for sgn in (+1.0, -1.0):
            d = np.zeros((conf.shape[0], 2 * D))
            d[:, k] = sgn * h
            x = oracle.retract(ro, np.concatenate([conf, np.zeros_like(conf)], axis=1), d)[:, :D]
            probes.append(mr.hinge_rows(oracle, model, ro, x, radius, cen, mr.EPSILON)[0])
        both = (probes[0] > 0) & (probes[1] > 0) & (err > 0)
        num = (probes[0] - probes[1]) / (2 * h)
        rows += int(both.sum())
        worst = max(worst, float(np.abs(num - H[..., k])[both].max()))
    print(f"{name}: {rows} active (row, coordinate)s, max |numeric - analytic| {worst:.2e}")
    assert rows > 0 and (err == 0).any()           # both branches of the hinge occur
    assert worst <= 1e-6


@pytest.mark.parametrize("k", [3, 5])
def test_reference_loop_reproduces_the_oracle_when_the_spheres_are_far_away(oracle, scen, k):
    p, mv, ro, so = scen
    q = copy.deepcopy(p)
    q.setting.fixed_iterations = k
    far = dict(mv, centers=mv["centers"] + 100.0)
    x = mr.gauss_newton(oracle, ro, so, q, far, k)
    want = oracle.batch_optimize(ro, so, q.setting, *mr._args(q), q.init)
    assert list(want["iters"]) == [k] * q.B
    assert np.array_equal(x.view(np.int64), want["traj"].view(np.int64))


def test_the_scenario_separates(oracle, scen):
    """from the reference alone: a row is in contact (clearance + epsilon < 0) without the factor, every row keeps
    0.05 with it; and the reference's own sensitivity to a 2-ulp perturbation of init stays below 1e-7"""
    p, mv, ro, so = scen
    without = mr.gauss_newton(oracle, ro, so, p, None, mr.ITERS)
    with_ = mr.gauss_newton(oracle, ro, so, p, mv, mr.ITERS)
    a = mr.support_clearance(oracle, p.model, ro, without, mv["radius"], mv["centers"], mv["epsilon"]) + mv["epsilon"]
    b = mr.support_clearance(oracle, p.model, ro, with_, mv["radius"], mv["centers"], mv["epsilon"]) + mv["epsilon"]
    nudged = p.init * (1.0 + 2 * np.finfo(np.float64).eps)
    sens = np.abs(mr.gauss_newton(oracle, ro, so, p, mv, mr.ITERS, init=nudged) - with_).max()
    print(f"min clearance + epsilon without the factor {a}, with it {b}; 2-ulp self-sensitivity {sens:.1e}")
    assert (a < 0.0).any()
    assert (b >= 0.05).all()
    assert sens < 1e-7


def test_the_rule_for_worst_is_decided_in_the_gpu_inputs(oracle):
    """at most 10 % of the rows of the GPU cases have a runner-up within 1e-6 of the minimum"""
    close = rows = 0
    made = {}
    for name, (N, J), K in mr.CHECK_CASES:
        if K == 0:
            continue
        if name not in made:
            model = mr.check_models()[name]()
            made[name] = (model, oracle.robot(model))
        model, ro = made[name]
        traj = mr.check_traj(name, N)
        radius, centers = mr.spheres_near(oracle, model, ro, traj, K, 17 + K, mr.EPSILON)
        exp = mr.oracle_moving_score(oracle, model, ro, radius, centers, mr.EPSILON, mr.CHECK_DT, J, traj)
        close += mr.close_rows(exp)
        rows += traj.shape[0]
        assert (exp["moving_dense_cost"] > 0).any(), (name, N, J, K)
    print(f"{close} of {rows} rows have a runner-up within 1e-6")
    assert close <= 0.1 * rows


def test_sphere_positions_between_support_states():
    c = np.array([[[0.0, 0.0, 0.0], [1.0, 2.0, 4.0], [1.0, 2.0, 8.0]]])
    o = mr.sphere_positions(c, 3)
    assert o.shape == (1, 9, 3)
    assert np.array_equal(o[0, ::4], c[0])
    assert np.array_equal(o[0, 1], [0.25, 0.5, 1.0]) and np.array_equal(o[0, 6], [1.0, 2.0, 6.0])
    assert np.array_equal(mr.sphere_positions(c, 0), c)
