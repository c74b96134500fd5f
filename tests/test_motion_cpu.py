"""The motion limits (include/gpmp2mi.h "motion limits") on the CPU oracle alone: the definitions of
tests/motion_reference.py are what they claim to be, the gap the feature closes is there on the inputs the scoring work was
argued on, the inputs of tests/test_gpu_motion.py decide their `worst` comparisons, and the tolerance of the GPU test is
tight enough to catch a slip of 1e-6 in the interpolation.  No GPU, no product answers."""
import numpy as np
import pytest

import motion_reference as mr
import score_reference as ref
import self_reference as sr
from gpmp2_amd import scoring


@pytest.fixture(scope="module")
def wam(oracle):
    model = mr.models()["wam"]()
    return model, oracle.robot(model)


@pytest.fixture(scope="module")
def motivation(oracle):
    """the second WAM input of the issue solved on the oracle, with the obstacle scores and the motion scores"""
    p, J = ref.motivation_inputs()[1]
    ro, so = oracle.robot(p.model), ref.oracle_sdf(oracle, p.sdf_origin, p.sdf_cell, p.sdf_data)
    res = oracle.batch_optimize(ro, so.handle, p.setting, p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
    dt = ref.delta_t(p.setting)
    return dict(p=p, J=J, ro=ro, dt=dt, res=res, obstacle=ref.oracle_score(oracle, p.model, ro, so, dt, J, res["traj"]),
                motion=mr.oracle_motion_score(oracle, p.model, ro, mr.WAM_LIMITS, dt, J, res["traj"]))


def test_acceleration_formulas_agree_with_finite_differences_of_the_dense_velocity(oracle, wam):
    """the two closed forms against one-sided differences of the oracle's up-sampled velocity at the ends of every
    interval: the acceleration is linear in time, so the difference over one sample step is off by half a step of its
    slope and the error halves with the step"""
    model, _ = wam
    N, dt = 6, sr.DELTA_T
    t = mr.case_traj("wam", N, 2)
    a = mr.acceleration_ends(t, dt, 7).reshape(2, N, 2, 7)
    errs = []
    for J in (24, 49, 99):
        U = oracle.interpolate_traj(7, False, None, dt, J, t)
        v = U[:, :, 7:].reshape(2, -1, 7)
        h = dt / (J + 1)
        first = (v[:, 1::J + 1] - v[:, 0:-1:J + 1]) / h                  # (v(tau = h) - v(0)) / h of every interval
        last = (v[:, J + 1::J + 1] - v[:, J:-1:J + 1]) / h               # (v(dt) - v(dt - h)) / h
        errs.append(max(np.abs(first - a[:, :, 0]).max(), np.abs(last - a[:, :, 1]).max()))
    print("finite-difference error at J = 24, 49, 99:", errs, "largest |a|", np.abs(a).max())
    assert errs[0] > errs[1] > errs[2] and errs[2] < 0.02 * np.abs(a).max()
    assert 1.8 < errs[0] / errs[1] < 2.2 and 1.8 < errs[1] / errs[2] < 2.2      # first order in the step


def test_time_scale_is_the_factor_that_just_meets_the_rate_limits(oracle, motivation):
    """stretch delta_t by s = time_scale with the velocities divided by s: every ratio is then <= 1 and one is 1"""
    m = motivation
    p, J, dt, traj, e = m["p"], m["J"], m["dt"], m["res"]["traj"], m["motion"]
    _, _, _, _, ps = mr.expand(mr.WAM_LIMITS, 7)
    for b in range(0, p.B, 5):
        s = e["time_scale"][b]
        slow = traj[b:b + 1].copy()
        slow[:, :, 7:] /= s
        g = mr.oracle_motion_score(oracle, p.model, m["ro"], mr.WAM_LIMITS, dt * s, J, slow)
        three = np.array([g["vel_ratio"][0], np.sqrt(g["acc_ratio"][0]), g["point_speed"][0] / ps])
        assert (three <= 1.0 + 1e-12).all() and abs(three.max() - 1.0) < 1e-12, (b, s, three)
        assert abs(g["time_scale"][0] - 1.0) < 1e-12
        assert abs(g["pos_margin"][0] - e["pos_margin"][b]) < 1e-12          # the path is the same: time buys no range


def test_the_gap_is_there_on_the_motivation_input(motivation):
    m = motivation
    res, ob, e = m["res"], m["obstacle"], m["motion"]
    ok = scoring.eligible(res["final_error"], res["status"], ob["min_clearance"], ob["out_of_range"], 0.0, False)
    outside = e["pos_margin"] < 0
    print(f"eligible by the obstacle rule {ok.sum()}, outside the joint ranges {outside.sum()} (by up to "
          f"{-e['pos_margin'].min():.3f} rad), both {(ok & outside).sum()}; time_scale {e['time_scale'].min():.2f} .. "
          f"{e['time_scale'].max():.2f}, vel_ratio {e['vel_ratio'].min():.2f} .. {e['vel_ratio'].max():.2f}")
    assert (ok & outside).any()
    assert (e["vel_ratio"] > 1.0).all() and (e["time_scale"] > 1.0).all()
    assert e["invalid"].sum() == 0
    # the rule with the new conditions refuses them, and never picks another row than the rule without would allow
    plain = scoring.select_rule(res["final_error"], res["status"], ob["min_clearance"], ob["out_of_range"])
    asked = scoring.feasible_rule(res["final_error"], res["status"], ob["min_clearance"], ob["out_of_range"],
                                  pos_margin=e["pos_margin"], time_scale=e["time_scale"], motion_invalid=e["invalid"],
                                  required_pos_margin=0.0, max_time_scale=np.inf)
    assert asked[1] == plain[1] - (ok & outside).sum() and not outside[asked[0]] and ok[asked[0]]
    none = scoring.feasible_rule(res["final_error"], res["status"], ob["min_clearance"], ob["out_of_range"],
                                 pos_margin=e["pos_margin"], time_scale=e["time_scale"], motion_invalid=e["invalid"],
                                 max_time_scale=1.0)
    assert none == (-1, 0)


def test_feasible_rule_without_limits_is_select_rule(oracle, motivation):
    m = motivation
    res, ob = m["res"], m["obstacle"]
    free = mr.oracle_motion_score(oracle, m["p"].model, m["ro"], mr.NO_LIMITS, m["dt"], m["J"], res["traj"])
    assert np.isposinf(free["pos_margin"]).all() and (free["vel_ratio"] == 0).all() and (free["acc_ratio"] == 0).all()
    assert (free["time_scale"] == 0).all() and np.isfinite(free["point_speed"]).all() and (free["point_speed"] > 0).all()
    assert (free["worst"][:, :3] == -1).all() and (free["worst"][:, 3] >= 0).all()
    rng = np.random.default_rng(3)
    for trial in range(20):
        fe = res["final_error"].copy()
        fe[rng.integers(0, len(fe), 3)] = [np.nan, np.inf, fe.min() - 1.0]
        st = rng.integers(0, 5, len(fe))
        req, rir = float(rng.choice([-np.inf, 0.0, 0.02])), bool(trial % 2)
        a = scoring.select_rule(fe, st, ob["min_clearance"], ob["out_of_range"], req, rir)
        b = scoring.feasible_rule(fe, st, ob["min_clearance"], ob["out_of_range"], req, rir, pos_margin=free["pos_margin"],
                                  time_scale=free["time_scale"], motion_invalid=free["invalid"], required_pos_margin=0.0,
                                  max_time_scale=np.inf)
        assert a == b and a == scoring.feasible_rule(fe, st, ob["min_clearance"], ob["out_of_range"], req, rir)


@pytest.mark.parametrize("case", mr.GPU_CASES, ids=[mr.case_id(c) for c in mr.GPU_CASES])
def test_the_gpu_inputs_decide_their_worst_comparisons(oracle, case):
    """at most one row in eight of a case has a runner-up within the value tolerance of its extremum"""
    name, (N, J), B = case
    model = mr.models()[name]()
    e = mr.oracle_motion_score(oracle, model, oracle.robot(model), mr.case_limits(name), mr.case_dt(name), J,
                               mr.case_traj(name, N, B))
    rows = len(e["invalid"])
    assert e["invalid"].sum() == 0
    for c, kind in enumerate(mr.KINDS):
        skipped = int((~mr.decided(e, c)).sum())
        print(mr.case_id(case), kind, "rows skipped", skipped, "of", rows, "smallest gap", np.nanmin(e["gap"][:, c]))
        if c not in mr.SHARE_EXEMPT.get(name, ()):
            assert skipped <= rows // 8, (kind, e["gap"][:, c])
    if name == "config5":      # the limits on the Pose2 coordinates would dominate if they were applied
        assert (e["worst"][:, 0, 1] >= 3).all() and (e["worst"][:, 2, 1] >= 3).all()
        assert (e["pos_margin"] > -1.0).all() and (e["acc_ratio"] < 1e3).all()


def test_the_motivation_input_decides_its_worst_comparisons(motivation):
    e = motivation["motion"]
    for c, kind in enumerate(mr.KINDS):
        assert (~mr.decided(e, c)).sum() <= len(e["invalid"]) // 8, (kind, e["gap"][:, c])


def test_the_constructed_rows_have_the_answers_they_were_built_for(oracle, wam):
    model, ro = wam
    S = model.nr_body_spheres()
    for N, J in ((8, 7), (12, 4), (12, 0)):
        Md = scoring.checked_states(N, J)
        uniform = dict(mr.WAM_ROUND)
        e = mr.oracle_motion_score(oracle, model, ro, uniform, sr.DELTA_T, J, mr.constructed_rows(N))
        assert tuple(e["worst"][0, 2]) == (0, 2) and tuple(e["worst"][1, 2]) == (2 * (N - 1) + 1, 4)
        assert tuple(e["worst"][2, 3]) == (Md - 1, S - 1) and e["gap"][2, 3] > 1e-3
        assert min(e["gap"][0, 2], e["gap"][1, 2]) > 1e-3
        if J == 0:     # the straight line: every state has the same velocity, every interval end acceleration 0
            assert tuple(e["worst"][3, 1]) == (0, 0) and tuple(e["worst"][3, 2]) == (0, 0)
            assert e["gap"][3, 1] == 0.0 and e["gap"][3, 2] == 0.0 and e["acc_ratio"][3] == 0.0
            assert e["vel_ratio"][3] == 0.25 / 2.0


def test_non_finite_coordinates_are_counted_and_enter_no_extremum(oracle, wam):
    model, ro = wam
    N, J = 6, 3
    t = mr.case_traj("wam", N, 3)
    clean = mr.oracle_motion_score(oracle, model, ro, mr.WAM_LIMITS, sr.DELTA_T, J, t)
    bad = t.copy()
    bad[1] = np.nan
    bad[2, 3, 2] = np.inf            # one joint of one support state: that coordinate of the 2 J + 1 states around it
    e = mr.oracle_motion_score(oracle, model, ro, mr.WAM_LIMITS, sr.DELTA_T, J, bad)
    assert e["invalid"][2] == (2 * J + 1) + 2 * J + 4 + (2 * J + 1) * 11 and np.isfinite(e["time_scale"][2])
    bad[2] = t[2]
    e = mr.oracle_motion_score(oracle, model, ro, mr.WAM_LIMITS, sr.DELTA_T, J, bad)
    Md, S = scoring.checked_states(N, J), model.nr_body_spheres()
    assert e["invalid"][1] == Md * 7 + Md * 7 + 2 * N * 7 + Md * S
    assert np.isposinf(e["pos_margin"][1]) and e["vel_ratio"][1] == 0 and e["acc_ratio"][1] == 0 and e["point_speed"][1] == 0
    assert (e["worst"][1] == -1).all()
    for k in mr.VALUES:
        assert np.array_equal(e[k][[0, 2]], clean[k][[0, 2]]), k
    fe = np.array([2.0, 1.0, 3.0])
    best, n = scoring.feasible_rule(fe, None, np.ones(3), None, pos_margin=e["pos_margin"], time_scale=e["time_scale"],
                                    motion_invalid=e["invalid"], required_pos_margin=-np.inf, max_time_scale=np.inf)
    assert best == 0 and n == 2


def test_a_slip_of_1e_6_in_the_interpolation_exceeds_the_cap(oracle, motivation):
    """the tolerance of tests/test_gpu_motion.py catches a relative mistake of 1e-6 in the interpolation time (every
    output whose extremum sits between two support states moves by more than CAP) and in the coefficient 6 of the
    acceleration formulas"""
    m = motivation
    p, J, dt, t = m["p"], m["J"], m["dt"], m["res"]["traj"]
    args = (oracle, p.model, m["ro"], mr.WAM_LIMITS, dt, J, t)
    good = mr.motion_from_states(*args, mr.hermite_states(t, dt, J, 7))
    assert max(mr.err(good[k], m["motion"][k]).max() for k in mr.VALUES) < mr.K * mr.FLOOR * 8   # the closed form is the GP mean
    bad = mr.motion_from_states(*args, mr.hermite_states(t, dt, J, 7, slip=1e-6))
    bad_acc = mr.motion_from_states(*args, mr.hermite_states(t, dt, J, 7), c6=6.0 * (1 + 1e-6))
    between = good["worst"][:, :, 0] % (J + 1) != 0            # [B][4]: the extremum is at an interpolated state
    for c, kind in ((0, "pos_margin"), (1, "vel_ratio"), (3, "point_speed")):
        rows = np.flatnonzero(between[:, c])
        moved = mr.err(bad[kind], good[kind])
        print(kind, "rows with the extremum between support states", rows.size, "smallest move", moved[rows].min() if rows.size else None)
        assert rows.size >= 3 and (moved[rows] > mr.CAP).all(), (kind, moved[rows])
    # time_scale follows the term that sets it: the velocity ratio, the acceleration or the point speed
    ps = mr.expand(mr.WAM_LIMITS, 7)[4]
    by_vel = (good["time_scale"] == good["vel_ratio"]) & between[:, 1]
    by_speed = (good["time_scale"] == good["point_speed"] / ps) & between[:, 3]
    by_acc = good["time_scale"] == np.sqrt(good["acc_ratio"])
    print("time_scale set by velocity / point speed / acceleration in", by_vel.sum(), by_speed.sum(), by_acc.sum(), "rows")
    assert (by_vel | by_speed).sum() >= 3
    assert (mr.err(bad["time_scale"], good["time_scale"])[by_vel | by_speed] > mr.CAP).all()
    assert (mr.err(bad_acc["time_scale"], good["time_scale"])[by_acc] > mr.CAP).all()
    assert (mr.err(bad_acc["acc_ratio"], good["acc_ratio"]) > mr.CAP).all()
    assert mr.CAP >= mr.K * mr.FLOOR
