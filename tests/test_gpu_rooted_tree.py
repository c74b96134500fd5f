"""The rooted cyclic-reduction tree of the one-tile path (cr_schedule.h crr_*: blocks v = state + 1, no block 0, the top
level inside the chain) on the GPU, for every shape of that tree.

One optimizer step per case, held to its backward error on the ORACLE's normal equations (tests/backward_error.py) with
the bound of tests/test_gpu_step_backward_error.py -- min(max(K eta_oracle, U_FLOOR), CAP), the rule written down in
profiles/step_backward_error.txt.  The lengths N cover a full tree (N + 1 = 2^k), one block over and under it, the top
level inside k_assemble's reach (N + 1 < 8: level 4 is the top, N + 1 < 4: level 2 is and is not fused), a first group
of three blocks (always) and a last group of one or two, for a planar 2-link arm and for the WAM, B = 3.  From N = 16 on
the step is finished either at the head of the next linearization (fused finish) or by k_finish_step
(no_fused_finish): the two must agree bit for bit.  LM and Dogleg take k_solve_step / k_finish_trial instead of
k_gn_step_cr.  Whole plans are then held to the parity contract (tests/parity_bound.py).

The oracle's linearization and its own step are computed once per (robot, N, optimizer) and shared by the forms.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import gpmp2_amd as g
from backward_error import eta_rows, one_step_setting, step_of
from gpmp2_amd import datasets, problems
from gpmp2_amd.settings import TrajOptimizerSetting
from gpmp2_amd.trajutils import initArmTrajStraightLine
from parity_bound import check_contract
from test_gpu_step_backward_error import ORACLE_CLEAN, bound

pytestmark = pytest.mark.gpu

B = 3
TREE_SHAPES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 14, 15, 16, 17, 30, 31, 32, 33, 62, 63, 64]
TRIAL_SHAPES = [2, 15, 16, 33]      # LM, Dogleg: k_solve_step (and k_finish_trial from N = 16 on)
PLAN_SHAPES = [15, 16, 33]
WIDE_RADIUS = 1e6                   # Dogleg: the first step is then the full Newton step


def _args(p):
    return p.start_conf, p.start_vel, p.end_conf, p.end_vel


def _wam(N, opt="GN"):
    return problems.wam_restarts(B=B, total_step=N, obs_check_inter=2, opt=opt, sdf="40")


def _planar2(N, opt="GN"):
    """a planar arm of two links with a sphere on each (so that its plans take the four-wavefront linearization and,
    from N = 16 on, the fused finish), between two obstacles"""
    D = 2
    arm = g.Arm(D, [0.9 / D] * D, [0.0] * D, [0.0] * D)
    model = g.ArmModel(arm, [g.BodySphere(l, 0.05, (-0.45 / D, 0, 0)) for l in range(D)])
    d = datasets.generate2Ddataset("TwoObstaclesDataset")
    fld = datasets.signedDistanceField2D(d.map, d.cell_size)
    st = TrajOptimizerSetting(D)
    st.set_total_step(N); st.set_total_time(3.0); st.set_obs_check_inter(2); st.set_cost_sigma(0.1); st.set_epsilon(0.2)
    st.set_conf_prior_model(1e-3); st.set_vel_prior_model(1e-3); st.set_Qc_model(np.eye(D)); st.set_max_iter(12)
    {"GN": st.setGaussNewton, "LM": st.setLM, "DOGLEG": st.setDogleg}[opt]()
    rng = np.random.default_rng(42)
    start = np.zeros((B, D))
    end = np.linspace(0.3, 0.9, D)[None] + 0.2 * rng.normal(size=(B, D))
    init = np.stack([initArmTrajStraightLine(start[b], end[b], N) for b in range(B)])
    z = np.zeros((B, D))
    return problems.Problem(f"planar arm, {D} joints", model, [d.origin_x, d.origin_y], d.cell_size, fld, st, start, z,
                            end, z.copy(), init)


ROBOTS = {"planar2": _planar2, "wam": _wam}
_oracle = None


@functools.lru_cache(maxsize=None)
def reference(robot, N, opt):
    """the problem, its one-step setting, and the oracle's H, g and own eta at the initial point"""
    p = ROBOTS[robot](N, opt)
    st = one_step_setting(p.setting, opt)
    if opt == "DOGLEG":
        st.dogleg_delta_initial = WIDE_RADIUS
    ro, so = _oracle.robot(p.model), _oracle.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    Hd, Ho, gr, _ = _oracle.linearize(ro, so, st, *_args(p), p.init)
    lam = st.lm_lambda_initial if opt == "LM" else 0.0
    dxo, reso = step_of(_oracle, p.init, False, ro, so, st, *_args(p))
    assert list(reso["iters"]) == [1] * B
    eta_oracle = float(eta_rows(Hd, Ho, gr, dxo, lam).max())
    # (for LM also the proof that the oracle accepted its first trial, for Dogleg that its step was the Newton step)
    assert eta_oracle <= ORACLE_CLEAN, (robot, N, opt, eta_oracle)
    return p, st, (Hd, Ho, gr, lam), eta_oracle


def one_step(engine, robot, N, opt, forms):
    """-> the step the plan took, the trajectory it returned, the kernels it launched"""
    p, st, _, _ = reference(robot, N, opt)
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pl = engine.plan(r, s, st, B, forms)
    try:
        pl.enable_timing(True)
        pl.set_problem(*_args(p), p.init)
        pl.optimize()
        launches = {k: v["launches"] for k, v in pl.timing().items()}
        dx, after = step_of(pl, p.init, False)
        assert list(after["iters"]) == [1] * B, list(after["iters"])
        if opt == "LM":         # the first trial was accepted: lambda went down one rung, once
            for b in range(B):
                assert pl.debug_scalars(b)["radius"] == st.lm_lambda_initial / st.lm_lambda_factor, b
        if opt == "DOGLEG":     # the step is the Newton step
            for b in range(B):
                sc = pl.debug_scalars(b)
                assert abs(sc["xnorm"] ** 2 - sc["nn"]) <= 1e-12 * sc["nn"], (b, sc)
    finally:
        pl.close()
    assert np.abs(dx).reshape(B, -1).max(axis=1).min() > 1e-6, "a trajectory did not move: nothing to measure"
    return dx, after["traj"].copy(), launches


def held_to_bound(label, robot, N, opt, dx):
    _, _, (Hd, Ho, gr, lam), eta_oracle = reference(robot, N, opt)
    eta_gpu = eta_rows(Hd, Ho, gr, dx, lam)
    lim = bound(eta_oracle)
    print(f"{label}: eta_gpu {eta_gpu.max():.2e} (trajectory {int(eta_gpu.argmax())}), eta_oracle {eta_oracle:.2e}, "
          f"bound {lim:.2e}")
    assert eta_gpu.max() <= lim, f"{label}: eta_gpu = {eta_gpu.max():.3e}, eta_oracle = {eta_oracle:.3e}, bound {lim:.3e}"


@pytest.fixture(autouse=True)
def _share_oracle(oracle):
    global _oracle
    _oracle = oracle


@pytest.mark.parametrize("N", TREE_SHAPES)
@pytest.mark.parametrize("robot", list(ROBOTS))
def test_gauss_newton_step_of_every_tree_shape(engine, robot, N):
    dx, traj, launches = one_step(engine, robot, N, "GN", None)
    assert launches.get("assemble", 0) >= 1 and launches.get("gn_step_cr", 0) >= 1, launches
    assert "solve_step" not in launches and "finish_step" not in launches, launches     # N >= 16: the fused finish
    held_to_bound(f"{robot} N={N} GN", robot, N, "GN", dx)
    if N >= 16:
        dx2, traj2, launches2 = one_step(engine, robot, N, "GN", {"no_fused_finish": 1})
        assert launches2.get("finish_step", 0) >= 1, launches2
        held_to_bound(f"{robot} N={N} GN no_fused_finish", robot, N, "GN", dx2)
        assert np.array_equal(traj, traj2), (robot, N, np.abs(traj - traj2).max())


@pytest.mark.parametrize("N", TRIAL_SHAPES)
@pytest.mark.parametrize("opt", ["LM", "DOGLEG"])
@pytest.mark.parametrize("robot", list(ROBOTS))
def test_trial_step_of_lm_and_dogleg(engine, robot, opt, N):
    dx, _, launches = one_step(engine, robot, N, opt, None)
    assert launches.get("assemble", 0) >= 1 and launches.get("solve_step", 0) >= 1 and "gn_step_cr" not in launches, launches
    if opt == "DOGLEG":
        assert launches.get("ghg", 0) >= 1, launches
    held_to_bound(f"{robot} N={N} {opt}", robot, N, opt, dx)
    if opt == "LM" and N >= 16:     # the split form next to the fused one: k_finish_trial
        dx2, _, launches2 = one_step(engine, robot, N, opt, {"no_fused_finish": 1})
        assert launches2.get("finish_trial", 0) >= 1, launches2
        held_to_bound(f"{robot} N={N} {opt} no_fused_finish", robot, N, opt, dx2)


@pytest.mark.parametrize("N", PLAN_SHAPES)
@pytest.mark.parametrize("opt", ["GN", "LM", "DOGLEG"])
def test_whole_plans_keep_the_parity_contract(engine, oracle, opt, N):
    """iteration counts and status identical to the oracle's, trajectories inside the contract"""
    check_contract(engine, oracle, _wam(N, opt), label=f"WAM N={N} {opt}")
