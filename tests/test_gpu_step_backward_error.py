"""One step of every solver form a plan can take, held to its backward error on the normal equations.

The end-to-end parity tests compare trajectories after Gauss-Newton has converged, and Gauss-Newton corrects a slightly
wrong step by itself: an elimination that is off by 1e-10 moves one step by 3e-9 .. 4e-6 and the converged trajectory by
nothing.  Here every case takes ONE step on the GPU and measures eta (tests/backward_error.py: the residual of every
block row of H dx + g against the size of its terms, in long double) twice:

  * against the ORACLE's linearization at the same point -- the independent reference, and the one that gates;
  * against the engine's own `linearize` at that point, which k_export_normal_eq builds, not k_assemble / the wide or
    dense assemblers the step came from.  When the two disagree the assembly is at fault, not the solve; both are
    printed.

The bound is eta_gpu <= min(max(K * eta_oracle, U_FLOOR), CAP) with eta_oracle the oracle's own step of the same case,
computed here.  K and U_FLOOR come from one measured run of this file (profiles/step_backward_error.txt, written by
scripts/step_backward_error.py, states the rule); CAP = 1e-13 is a condition, not a measurement: it lies below the
3.8e-13 that the smallest injected 1e-10 error produces on the CPU (tests/test_backward_error_cpu.py), about 50 times
above the oracle's largest value, and above bandwidth * log2(N) * u ~ 3e-14 for these sizes.

Every case also asserts from the plan's own timing read-out that the kernel form it claims to cover was launched.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import pytest

import gpmp2_amd as g
from backward_error import eta_rows, is_lie, one_step_setting, step_of
from gpmp2_amd import datasets, problems
from gpmp2_amd.settings import TrajOptimizerSetting
from gpmp2_amd.trajutils import initArmTrajStraightLine

pytestmark = pytest.mark.gpu

CAP = 1e-13        # no case is admitted above this, whatever K * eta_oracle says
K = 64.0                  # next power of two above 4 x 11.66, the largest eta_gpu / eta_oracle of the measured run
U_FLOOR = 4 * 3.254e-15   # 4 x the largest eta_gpu of the measured run (both: the PR2, N = 5)
ORACLE_CLEAN = 1e-14   # the oracle's own step (tests/test_backward_error_cpu.py)

TREE_SHAPES = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 64, 65]   # test_every_tree_shape_of_the_cyclic_reduction


def bound(eta_oracle):
    return min(max(K * eta_oracle, U_FLOOR), CAP)


def _args(p):
    return p.start_conf, p.start_vel, p.end_conf, p.end_vel


# ---------------------------------------------------------------------------------------------- problems
def _wam(B, N, inter, prior_sigma=None):
    p = problems.wam_restarts(B=B, total_step=N, obs_check_inter=inter, opt="GN", sdf="40")
    if prior_sigma is not None:
        p.setting.set_conf_prior_model(prior_sigma)
        p.setting.set_vel_prior_model(prior_sigma)
    return p


def _planar(D):
    """the planar arms of test_every_block_width_of_the_one_tile_path: D joints, N = 21, three trajectories"""
    arm = g.Arm(D, [0.9 / D] * D, [0.0] * D, [0.0] * D)
    model = g.ArmModel(arm, [g.BodySphere(l, 0.05, (-0.45 / D, 0, 0)) for l in range(D)])
    d = datasets.generate2Ddataset("TwoObstaclesDataset")
    fld = datasets.signedDistanceField2D(d.map, d.cell_size)
    N, B = 21, 3
    st = TrajOptimizerSetting(D)
    st.set_total_step(N); st.set_total_time(3.0); st.set_obs_check_inter(2); st.set_cost_sigma(0.1); st.set_epsilon(0.2)
    st.set_conf_prior_model(1e-3); st.set_vel_prior_model(1e-3); st.set_Qc_model(np.eye(D)); st.set_max_iter(12)
    rng = np.random.default_rng(40 + D)
    start = np.zeros((B, D))
    end = np.linspace(0.3, 0.9, D)[None] + 0.2 * rng.normal(size=(B, D))
    init = np.stack([initArmTrajStraightLine(start[b], end[b], N) for b in range(B)])
    z = np.zeros((B, D))
    return problems.Problem(f"planar arm, {D} joints", model, [d.origin_x, d.origin_y], d.cell_size, fld, st, start, z,
                            end, z.copy(), init)


def _straight(p, N):
    D = p.setting.dof
    for i in range(N + 1):
        p.init[0, i, :D] = p.start_conf[0] * (N - i) / N + p.end_conf[0] * i / N
    p.init[0, :, D:] = (p.end_conf[0] - p.start_conf[0])[None, :] / 3.0
    return p


WIDE = {8: "arm8 (dof 8)", 9: "2arms 3+3 (dof 9)", 10: "mobile WAM (dof 10)", 11: "lift WAM (dof 11)"}


def _wide(dof, N):
    """The robots of test_gpu_robots._wide_models.  dof 8 is a fixed-base arm (joint-space ends, as in
    test_wide_robot_linearize_and_plans); the kernels that walk a fixed-base chain are instantiated for at most 8 joints,
    so 9, 10 and 11 are the Pose2 robots of that table, measured through the local coordinates."""
    from test_gpu_robots import _tree_problem, _wide_models
    model = _wide_models()[WIDE[dof]]
    assert model.dof() == dof
    p = _tree_problem(model, N=N, inter=2, opt="GN")
    if not is_lie(model):
        p.start_conf[0, :] = 0.1
        p.end_conf[0, :] = np.linspace(0.3, 0.9, dof)
        _straight(p, N)
    return p


def _pr2(N):
    """generateMobileArm('PR2') as in test_pr2_model_plans: dof 18.  (Dense plans are created for dof 17 and 18, but no
    robot of 17 is instantiated -- two 7-joint arms on a base without the lift are refused when the plan runs -- and no
    fixed-base arm is this wide: so dof 18, through the local coordinates.)"""
    from test_gpu_robots import _tree_problem
    p = _tree_problem(g.generateMobileArm("PR2"), N=N, inter=1, opt="GN")
    p.end_conf[0, 3] = 0.2                                       # lift
    p.end_conf[0, 4:] = np.tile(np.linspace(0.2, 0.8, 7), 2) * np.r_[np.ones(7), -np.ones(7)]
    return _straight(p, N)


def _config5(delta=None):
    p = problems.mobile_arm_config5()
    if delta is not None:
        p.setting.dogleg_delta_initial = delta
    return p


# ---------------------------------------------------------------------------------------------- cases
@dataclass
class Case:
    id: str
    make: object                    # () -> problems.Problem
    opt: str = "GN"
    forms: dict = None
    want: tuple = ()                # timing names that must have been launched
    absent: tuple = ()              # ... and that must not
    update: bool = False            # measure the step of plan.update(1) after a one-iteration optimize


def _one_tile_cases():
    for N in TREE_SHAPES:
        split = N >= 16                     # levels 4, 2, 1 of the back-substitution leave the step kernel
        make = lambda N=N: _wam(3, N, 2)
        yield Case(f"one-tile default N={N}", make, want=("assemble", "gn_step_cr"),
                   absent=("solve_step", "finish_step", "final_error"))           # N >= 16: finished in k_linearize_arm
        yield Case(f"one-tile no_fused_finish N={N}", make, forms={"no_fused_finish": 1},
                   want=("assemble", "gn_step_cr") + (("finish_step",) if split else ()), absent=("solve_step",))
        yield Case(f"one-tile generic_gn N={N}", make, forms={"generic_gn": 1}, want=("assemble", "solve_step", "decide"),
                   absent=("gn_step_cr", "finish_trial"))
        yield Case(f"one-tile no_early_stop N={N}", make, forms={"no_early_stop": 1},
                   want=("assemble", "gn_step_cr", "final_error"), absent=("solve_step",))


def _fused_back_substitution_cases():
    # The step of pass k is applied by the head of pass k + 1's k_linearize_arm (levels 4 / 2 / 1 + retract) when the plan
    # has the fused finish: lin_split 4 and N >= 16.  plan.update(1) from a read-back trajectory is such a run: its timing
    # shows two linearizations and no finish_step.  The other (lin_split, N) of the grid take k_finish_step (N >= 16) or
    # finish inside the step kernel (N < 16); they are measured all the same, and their timing must say so.
    # End-point priors of sigma 0.1 instead of the WAM's 1e-4: a first step puts the two end states on their priors, the
    # second moves them by 1e-7, and a step that small cannot be read back from values of order 1 -- one rounding of the
    # value, times the prior's 1e8, is the whole residual of those two block rows (the ORACLE's second step then measures
    # 7.8e-12, tests/test_backward_error_cpu.py).  With priors that leave the ends free to move it measures 3e-16 .. 8e-16.
    for ls in (1, 2, 4):
        for N in (9, 17, 33):
            fused, split = ls == 4 and N >= 16, N >= 16
            yield Case(f"update lin_split={ls} N={N}", lambda N=N: _wam(3, N, 2, 0.1), forms={"lin_split": ls}, update=True,
                       want=("assemble", "gn_step_cr") + (("finish_step",) if split and not fused else ()),
                       absent=("solve_step",) + (("finish_step",) if fused or not split else ()))


def _block_width_cases():
    for D in range(1, 8):
        yield Case(f"planar D={D} GN", lambda D=D: _planar(D), want=("assemble", "gn_step_cr"), absent=("solve_step",))
        yield Case(f"planar D={D} LM", lambda D=D: _planar(D), opt="LM", want=("assemble", "solve_step"),
                   absent=("gn_step_cr",))


def _wide_cases():
    for dof in (8, 9, 10, 11):
        for N in (10, 17, 35):
            tail = ("cr_level2_wide",) + (("cr_level4_wide", "finish_trial_wide") if N >= 16 else ())
            yield Case(f"wide dof={dof} N={N}", lambda dof=dof, N=N: _wide(dof, N),
                       want=("assemble_wide", "solve_step_wide") + tail, absent=("solve_dense", "assemble"))
            yield Case(f"wide dof={dof} N={N} wide_dense", lambda dof=dof, N=N: _wide(dof, N), forms={"wide_dense": 1},
                       want=("export_dense", "solve_dense"), absent=("assemble_wide", "solve_step_wide"))
    yield Case("wide mobile WAM (Pose2, dof 10) N=20", lambda: _wide(10, 20),
               want=("assemble_wide", "solve_step_wide", "cr_level2_wide", "cr_level4_wide", "finish_trial_wide"),
               absent=("solve_dense",))


def _dense_cases():
    for N in (5, 16, 21):
        yield Case(f"dense PR2 (dof 18) N={N}", lambda N=N: _pr2(N), want=("export_dense", "solve_dense"),
                   absent=("assemble_wide", "assemble"))


def _lie_cases():
    yield Case("lie one-tile config5 GN", _config5, want=("assemble", "gn_step_cr", "finish_step"), absent=("solve_step",))
    # radius far beyond |dx_n|: the first Dogleg step is the full Newton step (asserted from debug_scalars)
    yield Case("lie one-tile config5 Dogleg wide radius", lambda: _config5(1e6), opt="DOGLEG",
               want=("assemble", "ghg", "solve_step"), absent=("gn_step_cr",))


def _conditioning_cases():
    for N in (300, 600):      # cond(H) grows like N^4 here; eta must not
        yield Case(f"conditioning N={N}", lambda N=N: _wam(1, N, 1), want=("assemble", "gn_step_cr", "finish_step"),
                   absent=("solve_step",))


def _batch_cases():
    # 70 distinct trajectories: past one wavefront of trajectories and past the 64-restart grid
    yield Case("batch B=70 N=9", lambda: _wam(70, 9, 2), want=("assemble", "gn_step_cr"), absent=("solve_step",))


def all_cases():
    out = []
    for gen in (_one_tile_cases, _fused_back_substitution_cases, _block_width_cases, _wide_cases, _dense_cases,
                _lie_cases, _conditioning_cases, _batch_cases):
        out.extend(gen())
    assert len({c.id for c in out}) == len(out)
    return out


# ---------------------------------------------------------------------------------------------- one measurement
def measure(engine, oracle, case):
    """Runs the case -> dict(eta_gpu, eta_own, eta_oracle: the worst row of each; launches; B, N, dof).  Asserts what
    makes the case the case it claims to be (one accepted step, the kernels launched), not the bound."""
    p = case.make()
    st = one_step_setting(p.setting, case.opt)
    lie, B, N = is_lie(p.model), p.B, p.setting.total_step
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    ro, so = oracle.robot(p.model), oracle.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    lam = st.lm_lambda_initial if case.opt == "LM" else 0.0
    pl = engine.plan(r, s, st, B, case.forms)
    try:
        pl.enable_timing(True)
        pl.set_problem(*_args(p), p.init)
        pl.optimize()
        before = p.init
        if case.update:
            before = pl.result()["traj"].copy()        # the read-back values are what update starts from
            pl.update(1)
        launches = {k: v["launches"] for k, v in pl.timing().items()}
        # the oracle's linearization at the same point: the reference
        Hd, Ho, gr, _ = oracle.linearize(ro, so, st, *_args(p), before)
        near = None
        if lie:     # heading steps are read back modulo 2 pi: the branch is the one next to the reference solve
            near, ok = oracle.block_tridiag_solve(Hd + lam * np.eye(Hd.shape[-1]), Ho, -gr)
            assert list(ok) == [1] * B
        dx, after = step_of(pl, before, lie, near=near)
        assert list(after["iters"]) == [1] * B, list(after["iters"])
        if case.opt == "LM":       # the first trial was accepted: lambda went down one rung, once
            for b in range(B):
                assert pl.debug_scalars(b)["radius"] == st.lm_lambda_initial / st.lm_lambda_factor, b
        if case.opt == "DOGLEG":   # the step is the Newton step: |step|^2 == |dx_n|^2 to rounding
            for b in range(B):
                sc = pl.debug_scalars(b)
                assert abs(sc["xnorm"] ** 2 - sc["nn"]) <= 1e-12 * sc["nn"], (b, sc)
                assert sc["nn"] < st.dogleg_delta_initial ** 2
    finally:
        pl.close()
    for name in case.want:
        assert launches.get(name, 0) >= 1, (case.id, name, launches)
    for name in case.absent:
        assert name not in launches, (case.id, name, launches)
    if case.update:
        assert launches["linearize"] == 2 and launches["assemble"] == 1, launches
    assert np.abs(dx).reshape(B, -1).max(axis=1).min() > 1e-6, "a trajectory did not move: nothing to measure"
    dxo, reso = step_of(oracle, before, lie, ro, so, st, *_args(p), near=near)     # the yardstick's zero
    assert list(reso["iters"]) == [1] * B
    eta_oracle = eta_rows(Hd, Ho, gr, dxo, lam)
    # (for LM this is also the proof that the oracle accepted its first trial: one rung up eta is ~1e-2; for Dogleg
    # that its step was the Newton step)
    assert eta_oracle.max() <= ORACLE_CLEAN, (case.id, eta_oracle.max())
    eta_gpu = eta_rows(Hd, Ho, gr, dx, lam)
    own = engine.linearize(r, s, st, *_args(p), before)
    eta_own = eta_rows(own[0], own[1], own[2], dx, lam)
    return dict(eta_gpu=float(eta_gpu.max()), eta_own=float(eta_own.max()), eta_oracle=float(eta_oracle.max()),
                worst_traj=int(eta_gpu.argmax()), launches=launches, B=B, N=N, dof=p.setting.dof)


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id.replace(" ", "_")) for c in all_cases()])
def test_step_backward_error(engine, oracle, case):
    m = measure(engine, oracle, case)
    lim = bound(m["eta_oracle"])
    print(f"{case.id}: eta_gpu {m['eta_gpu']:.2e} (trajectory {m['worst_traj']}), against the engine's own linearize "
          f"{m['eta_own']:.2e}, eta_oracle {m['eta_oracle']:.2e}, bound {lim:.2e}")
    assert m["eta_gpu"] <= lim, (
        f"{case.id}: eta_gpu = {m['eta_gpu']:.3e} against the oracle's linearization (trajectory {m['worst_traj']}), "
        f"{m['eta_own']:.3e} against the engine's own; eta_oracle = {m['eta_oracle']:.3e}, bound {lim:.3e}.  "
        "Both large: the solve; only the first: the assembly.")


def test_every_solver_form_has_a_case():
    """the kernel names the cases claim, taken together, are the forms plans solve with"""
    claimed = set()
    for c in all_cases():
        claimed.update(c.want)
    assert {"assemble", "gn_step_cr", "finish_step", "solve_step", "final_error", "ghg", "assemble_wide", "cr_level2_wide",
            "cr_level4_wide", "solve_step_wide", "finish_trial_wide", "export_dense", "solve_dense"} <= claimed
    # the fused back-substitution: update runs with lin_split 4 and N >= 16, and the split form next to them
    upd = [c for c in all_cases() if c.update]
    assert sum("finish_step" in c.want for c in upd) == 4 and sum("finish_step" in c.absent for c in upd) == 5
