"""The SO(3) / SE(3) maps of the kernels against the exact maps (tests/lie3_reference.py: mpmath, 60 digits, differenced
Jacobians, the link's body Jacobian from exact forward kinematics), over the cases of tests/lie3_cases.py -- the angle
of between(des, link pose) from 0 over 1e-18 to pi - 1e-9, every switch of form at 0.99 and 1.01 times its value, about
+-x, +-y, +-z and two generic axes, four translations, the WAM at two configurations and a mobile manipulator:

  * workspace_prior_factor in orientation and in pose mode: err and H -- Log on SO(3) and SE(3), their derivatives;
  * path_score_traj at inter_step 1 (orientation) and 3 (pose) on targets whose consecutive relative rotations run
    through the same angles: max_rot_dev, max_pos_dev, support_cost, dense_cost -- Exp of tau Log between two targets;
  * targets at exactly pi, compared on the group; targets whose rotation block is a float32 rounding: finite.

The oracle is a restatement of the same forms and cannot referee them; the exact maps do.  The gate follows
tests/test_gpu_pose2_maps.py: for every case and output
    e_gpu <= min(max(K * e_oracle, FLOOR), CAP),   e = max |got - exact| / scale   (tests/lie3_cases.py)
with e_oracle the oracle's error on the same case, computed here.  K and FLOOR come from one measured run
(profiles/lie3_maps_error.txt, written by scripts/lie3_maps_error.py, states the rule); CAP = 1e-12 is a condition:
double-precision prototypes of the forms reach 7e-16 (tests/test_lie3_reference_cpu.py) and every defect of GTSAM 4.0's
expressions exceeds it where it matters.

Two more tests guard that the fused kernels take the same code as the factor entry point: a WAM plan's linearization
with a workspace pose factor and a path at such angles, and the batched IK from seeds half a turn away from their
target."""
from __future__ import annotations

import copy
import math

import numpy as np
import pytest

import ik_reference as ik
import lie3_cases as lc
import lie3_reference as ref
import path_reference as pr

pytestmark = pytest.mark.gpu

CAP = lc.CAP
K = 32.0               # next power of two above 4 x 6.746, the largest e_gpu / e_oracle of the measured run (pose.err)
FLOOR = 4 * 8.945e-16  # 4 x the largest e_gpu among the cases with e_oracle < 1e-16 of the measured run (rot.err)


@pytest.fixture(scope="module")
def measured(engine, oracle):
    out = []
    for impl in (engine, oracle):
        h = lc.handles(impl)
        e = lc.measure(impl, h)
        e.update(lc.measure_path(impl, h))
        out.append(e)
    return out


@pytest.mark.parametrize("group", lc.GROUPS)
def test_gpu_maps_against_the_exact_maps(measured, group):
    e_gpu, e_orc = measured[0][group], measured[1][group]
    band = lc.case_bands(group)
    for k, name in enumerate(lc.BANDS):
        if (band == k).any():
            print(f"{group} {name}: e_gpu {e_gpu[band == k].max():.2e}  e_oracle {e_orc[band == k].max():.2e}")
    lim = np.minimum(np.maximum(K * e_orc, FLOOR), CAP)
    bad = np.flatnonzero(e_gpu > lim)
    worst = bad[np.argmax(e_gpu[bad])] if bad.size else -1
    assert bad.size == 0, (f"{group}: {bad.size} of {e_gpu.size} cases above the bound; the worst, case {worst} (band "
                           f"{lc.BANDS[band[worst]]}): e_gpu = {e_gpu[worst]:.3e}, e_oracle = {e_orc[worst]:.3e}")


def test_gpu_at_exactly_pi_on_the_group(engine):
    """|omega| within 4 ulp of pi and Exp(omega) the nearest rotation of Rd^T Rm to CAP: at pi the two signs of omega are
    one rotation, so omega itself is not compared"""
    for (ulps, d), case in zip(lc.measure_pi(engine, lc.handles(engine)), lc.pi_cases()):
        print(f"mode {case[1]}: | |omega| - pi | = {ulps:.0f} ulp, max |Exp(omega) - Rrel| = {d:.2e}")
        assert ulps <= 4 and d <= CAP


def test_gpu_stays_finite_on_targets_that_are_not_quite_rotations(engine):
    for (ok, e_err, e_H), case in zip(lc.measure_nonortho(engine, lc.handles(engine)), lc.nonortho_cases()):
        print(f"mode {case[1]} theta {case[3]:.10g}: from the exact maps on the polar factor err {e_err:.1e} H {e_H:.1e}")
        assert ok


# ------------------------------------------------------------------------------------------------ in a plan
PLAN_THETAS = [0.0, 1e-6, 1e-4, math.pi - 1e-6]


def _targets(poses, axes, t=(0.02, -0.01, 0.015)):
    """des[i] = poses[i] * (Exp(theta_i a_i), t)^-1 in mpmath, rounded: between(des[i], poses[i]) is theta_i about a_i"""
    out = []
    for i, T in enumerate(poses):
        a = ref.M(axes[i % len(axes)])
        off = (ref.Exp([ref.mpf(PLAN_THETAS[i % 4]) * x for x in a]), ref.vec(ref.M(t)))
        out.append(ref.rounded(ref.compose(ref.pose_of(T), ref.inverse(off))))
    return np.array(out)


def test_plan_linearize_at_the_angles_where_the_forms_changed(engine, oracle):
    """A WAM plan, N = 8, B = 3, with a workspace pose factor on one state and a pose path on all, whose targets sit at
    theta = 0, 1e-6, 1e-4 and pi - 1e-6 from row 0's link poses (rows 1 and 2 are generic).  plan linearize and
    graph_error against the oracle at the tolerance of tests/test_gpu_pose2_linearize_small_headings.py.  This guards
    that the fused kernels take the same code as the factor entry point, which the exact-value gate above goes through;
    it says nothing about the values."""
    from gpmp2_amd import problems
    p = problems.wam_restarts(B=3, total_step=8, obs_check_inter=2, sdf="40", opt="LM")
    link, N = 6, 8
    traj = p.init + 0.05 * np.random.default_rng(3).normal(size=p.init.shape)
    ro = oracle.robot(p.model)
    poses = pr.link_poses(oracle, ro, traj[0, :, :7], link)
    des = _targets(poses, [lc.AXES[6], lc.AXES[1], lc.AXES[5]])
    e0, _ = pr.rows(oracle, ro, pr.POSE, link, traj[0, :, :7], des)
    got = np.linalg.norm(e0[:, :3], axis=1)
    assert np.abs(got - np.array([PLAN_THETAS[i % 4] for i in range(N + 1)])).max() <= 1e-9
    q = copy.deepcopy(p)
    q.setting.add_workspace_prior(pr.POSE, link, des[3], 0.05, 3, 3)          # pi - 1e-6 on row 0's state 3
    q.setting.set_workspace_path(pr.POSE, link)
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    so = oracle.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pl = engine.plan(r, s, q.setting, 3)
    pl.set_problem(*pr._args(q), q.init)
    sigma = np.full(N + 1, 0.05)
    pl.set_workspace_path(des, sigma)
    a = pl.linearize(traj)
    native = copy.deepcopy(p)
    native.setting.add_workspace_prior(pr.POSE, link, des[3], 0.05, 3, 3)
    b = pr.linearize(oracle, ro, so, native, traj, dict(mode=pr.POSE, link=link, des=des, sigma=sigma))
    for name, x, y in zip(("Hd", "Ho", "g"), a[:3], b[:3]):
        print(f"{name}: max |gpu - oracle| = {np.abs(x - y).max():.2e}, max |oracle| = {np.abs(y).max():.2e}")
        np.testing.assert_allclose(x, y, atol=1e-9 * np.abs(y).max())
    np.testing.assert_allclose(a[3], b[3], rtol=1e-9)
    np.testing.assert_allclose(pl.graph_error(traj), b[3], rtol=1e-9)
    pl.close()


# ------------------------------------------------------------------------------------------------ IK
IK_SEEDS = [lc.CONFIGS[0][2], lc.CONFIGS[1][2]]


def ik_case(oracle):
    """WAM, pose mode: pose g = the seed's own link pose turned by pi - 1e-6 (g < 6) or pi - 1e-9 (g >= 6) about
    +-x, +-y, +-z and moved by a few centimetres; row 0 of a pose is that seed, row 1 the same seed a little off.
    G * M = 24 rows."""
    import gpmp2_amd as g
    model = g.generateArm("WAMArm")
    o = ik.Opts(mode=ik.POSE, link=6, down=ik.WAM_DOWN, up=ik.WAM_UP)
    poses, seeds = [], []
    for n in range(12):
        q = np.array(IK_SEEDS[n % 2])
        th = math.pi - (1e-6 if n < 6 else 1e-9)
        T = ref.fk(model.fk_model(), q, 6)[0]
        off = (ref.Exp([ref.mpf(th) * x for x in ref.M(lc.AXES[n % 6])]), ref.vec(ref.M((0.05, -0.1, 0.08))))
        poses.append(ref.rounded(ref.compose(T, ref.inverse(off))))
        seeds.append([q, q + 0.02 * np.sin(np.arange(7) + n)])
    return ik.Case("wam_pose_half_turn", model, o, 12, 2, 0, 0, np.array(poses), np.array(seeds))


def test_ik_from_seeds_half_a_turn_from_the_target(engine, oracle):
    """status, iteration count and answer against tests/ik_reference.py by the rule of tests/test_gpu_ik.py; the seeds'
    orientation error is pi - 1e-6 and pi - 1e-9 as built, and no seed ends INVALID"""
    import test_gpu_ik as tik
    case = ik_case(oracle)
    ro = oracle.robot(case.model)
    for i in range(case.G):
        e, _ = oracle.workspace_prior_factor(ro, ik.POSE, 6, case.poses[i], case.seeds[i, :1])
        assert abs(math.pi - np.linalg.norm(e[0, :3]) - (1e-6 if i < 6 else 1e-9)) <= 1e-12
    rf = ik.solve_all(oracle, ro, case.opts, case.poses, case.seeds)
    d_self, flips = ik.sensitivity(oracle, case, rf)
    assert not flips.any()                      # the condition under which rows are compared (tests/test_gpu_ik.py)
    m = tik.measure_case(engine, case, rf, d_self)
    n_diff = int(m["differ"].sum())
    over = m["both"] & ~m["differ"] & (m["e_gpu"] > tik.bound(m["d_self"]))
    print(f"rows {m['differ'].size}: status/iters differ on {n_diff}, converged on both {int(m['both'].sum())}, largest e_gpu "
          f"{m['e_gpu'].max():.3e}; iters {m['dev']['iters'].tolist()}")
    assert (m["dev"]["status"] != ik.INVALID).all() and (rf["status"] != ik.INVALID).all()
    assert n_diff <= tik.MISMATCH * m["differ"].size
    assert not over.any(), (m["e_gpu"][over], m["d_self"][over])
    tik._check_independent(oracle, case, m["dev"])
