"""Gauss-Newton fast driver: the step control decided BEFORE the normal equations are built.

k_linearize_arm leaves the graph error of every chunk of 64 evaluation points in three shares (obstacle, GP prior,
priors / limits); k_assemble and k_gn_step_cr both form the error from them and take the gpmp2::optimize decision with
one shared function, so a trajectory that stops in a pass builds and eliminates nothing in it.  The forced form
no_early_stop = 1 keeps the earlier order (the error summed over k_assemble's blocks, the decision in the step kernel
alone).  Every case compares the two:

  * traj, iters, status equal bit for bit -- nothing in the solve changes;
  * final_error and error_trace to rtol 1e-12: only the order of a sum of ~800 non-negative terms changes (n u ~ 9e-14;
    1e-12 is the tolerance tests/test_bench_outputs.py uses for final_error);
  * the on-run against the CPU oracle: identical iters and status, traj to 1e-6, per-iteration errors to 1e-9 relative.

Identical iters needs every convergence comparison to sit away from its threshold: each case computes that margin from
the oracle's error trace, on the CPU, and refuses a problem whose smallest margin is below 1e-9.
"""
import ctypes as C
from copy import deepcopy

import numpy as np
import pytest

from gpmp2_amd import problems
from gpmp2_amd._capi import dptr

pytestmark = pytest.mark.gpu

ON, OFF = None, {"no_early_stop": 1}
MARGIN = 1e-9


def _args(p):
    return p.start_conf, p.start_vel, p.end_conf, p.end_vel


def _margin(st, trace, iters):
    """Smallest distance of any comparison of the step control (gtsam::checkConvergence and the no-increase test of
    gpmp2::optimize, fed with the oracle's errors) from its threshold, relative where the comparison is."""
    m = np.inf
    for b in range(trace.shape[0]):
        e = trace[b, :int(iters[b]) + 1]
        assert np.isfinite(e).all(), (b, e)
        if st.error_tol > 0:
            m = min(m, np.abs(e - st.error_tol).min() / st.error_tol)
        for prev, new in zip(e[:-1], e[1:]):
            m = min(m, abs((prev - new) / prev - st.rel_thresh))           # relative decrease against rel_thresh
            m = min(m, abs((prev - new) - st.abs_error_tol) / max(prev, st.abs_error_tol))   # absolute decrease
            m = min(m, abs(new - prev) / prev)                            # new > prev: the rollback test
    return m


def _same_solve(on, off):
    for k in ("traj", "iters", "status"):
        np.testing.assert_array_equal(on[k], off[k], err_msg=k)
    np.testing.assert_allclose(on["final_error"], off["final_error"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(on["error_trace"], off["error_trace"], rtol=1e-12, atol=0, equal_nan=True)


def _against_oracle(on, ref, ref_trace):
    assert list(on["iters"]) == list(ref["iters"]), (list(on["iters"]), list(ref["iters"]))
    assert list(on["status"]) == list(ref["status"])
    np.testing.assert_allclose(on["traj"], ref["traj"], atol=1e-6)
    for b in range(len(ref["iters"])):
        k = int(ref["iters"][b]) + 1
        np.testing.assert_allclose(on["error_trace"][b, :k], ref_trace[b, :k], rtol=1e-9, atol=0, err_msg=f"row {b}")
    print("max rel. error of the per-iteration errors:",
          np.nanmax(np.abs(on["error_trace"] / ref_trace - 1.0)), "iters", list(on["iters"]))


def _both(engine, p, st):
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    return (engine.batch_optimize(r, s, st, *_args(p), p.init, forms=ON),
            engine.batch_optimize(r, s, st, *_args(p), p.init, forms=OFF))


def _case(engine, oracle, p, st, fixed=False):
    ro, so = oracle.robot(p.model), oracle.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    ref = oracle.batch_optimize(ro, so, st, *_args(p), p.init)
    if not fixed:
        m = _margin(st, ref["error_trace"], ref["iters"])
        print("smallest margin of a convergence comparison:", m)
        assert m >= MARGIN, f"a convergence comparison sits within {m:.1e} of its threshold: not a problem for this test"
    on, off = _both(engine, p, st)
    _same_solve(on, off)
    _against_oracle(on, ref, ref["error_trace"])
    return on, ref


def test_headline_settings_trajectories_stop_in_different_passes(engine, oracle):
    """N = 100, 5 sub-steps (13 chunks per trajectory), the small field: the restarts stop in several different passes."""
    p = problems.wam_restarts(B=12, total_step=100, obs_check_inter=5, opt="GN", sdf="40")
    on, _ = _case(engine, oracle, p, p.setting)
    assert len(set(on["iters"])) >= 3, list(on["iters"])


def test_total_step_not_a_multiple_of_8(engine, oracle):
    p = problems.wam_restarts(B=6, total_step=37, obs_check_inter=2, opt="GN", sdf="40")
    _case(engine, oracle, p, p.setting)


def test_obs_skip_first_state(engine, oracle):
    p = problems.wam_restarts(B=6, total_step=23, obs_check_inter=4, opt="GN", sdf="40")
    p.setting.obs_skip_first_state = True
    _case(engine, oracle, p, p.setting)


def test_fixed_iterations_closing_pass_launches_no_error_kernel(engine, oracle):
    """The closing pass of a fixed-iteration run has neither k_assemble nor k_error_parts: the plan's own timing shows no
    `final_error` launch with the form on, and one with it off."""
    p = problems.wam_restarts(B=6, total_step=64, obs_check_inter=3, opt="GN", sdf="40")
    st = deepcopy(p.setting)
    st.fixed_iterations = 3
    on, _ = _case(engine, oracle, p, st, fixed=True)
    assert list(on["iters"]) == [3] * p.B
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    launches = {}
    for name, forms in (("on", ON), ("off", OFF)):
        pl = engine.plan(r, s, st, p.B, forms)
        pl.enable_timing(True)
        pl.set_problem(*_args(p), p.init)
        pl.optimize()
        launches[name] = {k: v["launches"] for k, v in pl.timing().items()}
        pl.close()
    assert "final_error" not in launches["on"] and launches["on"]["assemble"] == 3, launches
    assert launches["off"]["final_error"] == 1 and launches["off"]["assemble"] == 3, launches


def _hinge(z, lo, hi, th):
    return np.maximum(0.0, np.maximum(lo + th - z, z - (hi - th)))


def test_position_and_velocity_limits_with_the_hinge_firing(engine, oracle):
    """Joint and velocity limits tight enough that both hinges are active at the initial values and on the way."""
    p = problems.wam_restarts(B=6, total_step=24, obs_check_inter=3, opt="GN", sdf="40")
    st, D = p.setting, 7
    conf, vel = p.init[:, :, :D], p.init[:, :, D:]
    lo, hi = conf.min(axis=(0, 1)), conf.max(axis=(0, 1))
    shrink = 0.1 * (hi - lo) + 0.01
    lo, hi = lo + shrink, hi - shrink
    vmax = 0.7 * np.abs(vel).max(axis=(0, 1)) + 0.01
    st.set_flag_pos_limit(True)
    st.set_flag_vel_limit(True)
    st.set_joint_pos_limits_down(lo)
    st.set_joint_pos_limits_up(hi)
    st.set_vel_limits(vmax)
    st.set_pos_limit_thresh(np.full(D, 0.01))
    st.set_vel_limit_thresh(np.full(D, 0.01))
    st.set_pos_limit_model(np.full(D, 0.05))
    st.set_vel_limit_model(np.full(D, 0.2))
    on, ref = _case(engine, oracle, p, st)
    for t in (p.init, ref["traj"]):
        assert (_hinge(t[:, :, :D], lo, hi, 0.01) > 0).any(axis=(1, 2)).all(), "position hinge inactive"
    assert (_hinge(p.init[:, :, D:], -vmax, vmax, 0.01) > 0).any(axis=(1, 2)).all(), "velocity hinge inactive"
    assert (on["iters"] >= 2).all(), list(on["iters"])


def test_fix_state_prior(engine, oracle):
    """A replanner state prior (gpmp2mi_plan_fix_state) is part of the misc share.  The oracle's entry point for such
    graphs returns no trace: the errors per iteration are its final errors after k = 1, 2, .. fixed iterations (Gauss-Newton
    is deterministic), and the error of the initial values is its graph error plus the prior's own 0.5 r^T W r."""
    p = problems.wam_restarts(B=4, total_step=20, obs_check_inter=4, opt="GN", sdf="40")
    st, D = p.setting, 7
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    ro, so = oracle.robot(p.model), oracle.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    b_fix, state = 1, 6
    conf = p.init[b_fix, state, :D] + 0.05
    vel = p.init[b_fix, state, D:] - 0.02
    w = 1.0 / st.conf_prior_sigma ** 2
    wv = 1.0 / st.vel_prior_sigma ** 2
    priors = [[] for _ in range(p.B)]
    priors[b_fix] = [dict(state=state, conf=conf, Wc=w * np.eye(D), vel=vel, Wv=wv * np.eye(D))]
    ref = oracle.batch_optimize_xp(ro, so, st, *_args(p), p.init, priors, [1] * p.B)
    e0 = oracle.graph_error(ro, so, st, *_args(p), p.init)
    e0[b_fix] += 0.5 * (w * 0.05 ** 2 * D + wv * 0.02 ** 2 * D)
    trace = np.full((p.B, st.max_iter + 1), np.nan)
    trace[:, 0] = e0
    fx = deepcopy(st)
    for k in range(1, int(ref["iters"].max()) + 1):
        fx.fixed_iterations = k
        ek = oracle.batch_optimize_xp(ro, so, fx, *_args(p), p.init, priors, [1] * p.B)["final_error"]
        rows = ref["iters"] >= k
        trace[rows, k] = ek[rows]
    m = _margin(st, trace, ref["iters"])
    print("smallest margin of a convergence comparison:", m)
    assert m >= MARGIN
    res = {}
    for name, forms in (("on", ON), ("off", OFF)):
        pl = engine.plan(r, s, st, p.B, forms)
        pl.set_problem(*_args(p), p.init)
        pl.fix_state(b_fix, state, conf, vel)
        pl.optimize()
        res[name] = pl.result()
        pl.close()
    _same_solve(res["on"], res["off"])
    _against_oracle(res["on"], ref, trace)
    np.testing.assert_allclose(res["on"]["final_error"], ref["final_error"], rtol=1e-9)
    # the prior holds: the state moved to the target
    np.testing.assert_allclose(res["on"]["traj"][b_fix, state, :D], conf, atol=1e-3)


def test_queue_of_three_rounds_against_batch_runs(engine, oracle):
    """3 B problems through B slots: fresh slots (iters == 0) enter at later passes and take the first-evaluation branch in
    both kernels.  Row for row the queue returns what batch runs of the same plan return, bit for bit, with the form on
    and with it off; on against off as everywhere; the on-run meets the oracle."""
    B = 4
    p = problems.wam_restarts(B=3 * B, total_step=16, obs_check_inter=3, opt="GN", sdf="40")
    st = p.setting
    rows = (*_args(p), p.init)
    ro, so = oracle.robot(p.model), oracle.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    ref = oracle.batch_optimize(ro, so, st, *rows)
    m = _margin(st, ref["error_trace"], ref["iters"])
    print("smallest margin of a convergence comparison:", m)
    assert m >= MARGIN
    assert len(set(ref["iters"])) > 1, list(ref["iters"])
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    res = {}
    for name, forms in (("on", ON), ("off", OFF)):
        pl = engine.plan(r, s, st, B, forms)
        q = pl.optimize_queue(*rows)
        parts = []
        for c0 in range(0, 3 * B, B):
            pl.set_problem(*[a[c0:c0 + B] for a in rows])
            pl.optimize()
            parts.append(pl.result())
        pl.close()
        batch = {k: np.concatenate([x[k] for x in parts]) for k in parts[0]}
        for k in ("traj", "iters", "status", "final_error"):
            np.testing.assert_array_equal(q[k], batch[k], err_msg=f"{name} {k}")
        assert np.array_equal(q["error_trace"], batch["error_trace"], equal_nan=True), name
        res[name] = q
    _same_solve(res["on"], res["off"])
    _against_oracle(res["on"], ref, ref["error_trace"])


def test_plan_with_extra_factors_falls_back_bit_for_bit(engine, oracle):
    """Workspace factors add their errors to the records behind the linearization, where the shares do not see them: such
    a plan keeps the earlier path, so forcing no_early_stop changes nothing at all."""
    p = problems.wam_restarts(B=4, total_step=20, obs_check_inter=4, opt="GN", sdf="40")
    st, N = p.setting, 20
    des = np.eye(4)
    des[:3, 3] = [0.3, 0.3, 0.5]
    st.add_workspace_prior(0, 6, des, 0.05, N // 2)
    on, off = _both(engine, p, st)
    for k in ("traj", "iters", "status", "final_error"):
        np.testing.assert_array_equal(on[k], off[k], err_msg=k)
    assert np.array_equal(on["error_trace"], off["error_trace"], equal_nan=True)
    ro, so = oracle.robot(p.model), oracle.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    ref = oracle.batch_optimize(ro, so, st, *_args(p), p.init)
    assert list(on["iters"]) == list(ref["iters"]) and list(on["status"]) == list(ref["status"])
    np.testing.assert_allclose(on["traj"], ref["traj"], atol=1e-6)


def test_the_build_of_the_stopping_pass_is_skipped(engine, oracle):
    """After a to-tolerance run the factor tiles of a trajectory tell which pass built them: the off-run rebuilt the
    level-1 / level-2 factors at the final values in the pass that only found out that the trajectory stops, the on-run
    kept those of the pass before.  So they differ for every trajectory that iterated, while the results are equal."""
    p = problems.wam_restarts(B=8, total_step=32, obs_check_inter=3, opt="GN", sdf="40")
    st, N = p.setting, 32
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    res, fac = {}, {}
    for name, forms in (("on", ON), ("off", OFF)):
        pl = engine.plan(r, s, st, p.B, forms)
        pl.set_problem(*_args(p), p.init)
        pl.optimize()
        res[name] = pl.result()
        f = np.zeros(p.B * (N + 1) * 768)
        engine._ck(engine.lib.gpmp2mi_plan_debug_read(pl.h.ptr, 1, dptr(f), C.c_long(f.size)))
        fac[name] = f.reshape(p.B, N + 1, 3, 256)
        pl.close()
    _same_solve(res["on"], res["off"])
    assert (res["on"]["iters"] >= 1).all(), list(res["on"]["iters"])
    odd = np.arange(1, N + 1, 2)               # level-1 blocks: written by k_assemble alone
    for b in range(p.B):
        assert np.isfinite(fac["on"][b]).all() and np.isfinite(fac["off"][b]).all()
        assert not np.array_equal(fac["on"][b, odd], fac["off"][b, odd]), f"trajectory {b}: the stopping pass was built"
