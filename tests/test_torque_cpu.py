"""tests/torque_reference.py pinned on the CPU with facts that do not depend on it, and the inputs of
tests/test_gpu_torque.py judged before a GPU sees them:
  (a) the textbook closed form of the planar two-link arm;
  (b) power balance along a smooth trajectory: tau . q' = d/dt (kinetic + potential energy), the energies formed from
      forward kinematics alone;
  (c) the mass matrix recovered column by column from unit accelerations is symmetric and positive definite;
  (d) torque_ratio <= 1  <=>  torque_time_scale <= 1 (given static_ratio < 1);
  (e) a trajectory restated with dt' = c dt and velocities / c has torque_time_scale / c;
  (f) four planted slips each move some torque of the GPU test inputs by more than 100 CAP;
and the link frames against the oracle's forward kinematics, the reference's own error against the truth in
np.longdouble (e_cpu <= CAP / 8 on the GPU inputs), the share of rows whose `worst` is left undecided, and the constructed
rows' known answers."""
import numpy as np
import pytest

import torque_reference as tr

ARMS = ("one", "two", "wam", "arm8")


@pytest.fixture(scope="module")
def made(oracle):
    out = {}
    for name in ARMS:
        model = tr.models()[name]()
        out[name] = (model, oracle.robot(model), tr.case_table(name))
    return out


def _random_states(D, M, seed, vmax=2.0, amax=20.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-2, 2, (M, D)), rng.uniform(-vmax, vmax, (M, D)), rng.uniform(-amax, amax, (M, D))


def test_link_frames_are_the_oracles(oracle, made):
    for name in ARMS:
        model, ro, _ = made[name]
        q, _, _ = _random_states(model.dof(), 20, 1)
        R, t, _, _ = tr.link_frames(model.fk_model(), q)
        poses, _ = oracle.forward_kinematics(ro, q)
        assert np.abs(R - poses[:, :, :3, :3]).max() < 1e-13 and np.abs(t - poses[:, :, :3, 3]).max() < 1e-13, name


def test_a_planar_two_link_closed_form(made):
    model, _, table = made["two"]
    q, qd, qdd = _random_states(2, 200, 2)
    want = tr.planar_two_link(table, q, qd, qdd)
    got64 = tr.inverse_dynamics(model.fk_model(), table, q, qd, qdd)
    gotld = tr.inverse_dynamics(model.fk_model(), table, q, qd, qdd, np.longdouble)
    assert tr.err(got64, want).max() < 1e-13
    if np.finfo(np.longdouble).eps < 1e-18:
        assert tr.err(gotld, want).max() < 1e-17


@pytest.mark.parametrize("name", ["two", "wam", "arm8"])
def test_b_power_balance(made, name):
    model, _, table = made[name]
    arm, D, ld = model.fk_model(), model.dof(), np.longdouble
    rng = np.random.default_rng(3)
    q0, A, om, ph = rng.uniform(-1, 1, D), rng.uniform(0.2, 0.8, D), rng.uniform(0.5, 2.0, D), rng.uniform(0, 6, D)

    def state(t):
        t = np.asarray(t, dtype=ld).reshape(-1, 1)
        s, c = np.sin(om.astype(ld) * t + ph.astype(ld)), np.cos(om.astype(ld) * t + ph.astype(ld))
        return q0 + A * s, A * om * c, -A * om * om * s
    t = np.linspace(0.0, 3.0, 25).astype(ld)
    h = ld(1e-3)
    E = lambda tt: tr.energy(arm, table, *state(tt)[:2])
    dE = (-E(t + 2 * h) + 8 * E(t + h) - 8 * E(t - h) + E(t - 2 * h)) / (12 * h)      # fourth order: error ~ h^4
    q, qd, qdd = state(t)
    for dtype, tol in ((ld, 1e-9), (np.float64, 1e-9)):
        power = (tr.inverse_dynamics(arm, table, q, qd, qdd, dtype) * qd).sum(axis=1)
        assert np.abs(power - dE).max() <= tol * max(1.0, float(np.abs(dE).max())), (name, dtype)
    for slip in ("no_wdot_product", "com_frame"):          # the balance notices a planted mistake
        power = (tr.inverse_dynamics(arm, table, q, qd, qdd, ld, slip) * qd).sum(axis=1)
        if name != "two" or slip == "com_frame":
            assert np.abs(power - dE).max() > 1e-4, (name, slip)


@pytest.mark.parametrize("name", ARMS)
def test_c_mass_matrix_is_symmetric_positive_definite(made, name):
    model, _, table = made[name]
    arm, D = model.fk_model(), model.dof()
    q, _, _ = _random_states(D, 10, 4)
    zero = np.zeros_like(q)
    g = tr.inverse_dynamics(arm, table, q, zero, zero, np.longdouble)
    M = np.stack([tr.inverse_dynamics(arm, table, q, zero, np.eye(D)[k] + zero, np.longdouble) - g for k in range(D)], axis=2)
    assert np.abs(M - np.swapaxes(M, 1, 2)).max() < 1e-15
    assert (np.linalg.eigvalsh(M.astype(np.float64)) > 0).all()


def _gpu_inputs(made, oracle):
    for case in tr.GPU_CASES:
        name, (N, J), B = case
        model, ro, table = made[name]
        yield case, model, table, tr.case_dt(N), J, tr.case_traj(name, N, B)


def test_d_ratio_and_time_scale_agree_on_what_is_executable(made, oracle):
    seen = set()
    for case, model, table, dt, J, traj in _gpu_inputs(made, oracle):
        D = model.dof()
        for factor, c in ((0.5, 1.0), (1.0, 1.0), (4.0, 1.0), (1.0, 0.5), (1.0, 0.3), (4.0, 0.3)):
            t = dict(table, torque=table["torque"] * factor)
            fast = traj.copy()                    # the same path run in c times the duration
            fast[:, :, D:] /= c
            s = tr.reference_torque_score(oracle, model, t, dt * c, J, fast)
            ok = s["static_ratio"] < 1
            assert np.array_equal(s["torque_ratio"][ok] <= 1, s["torque_time_scale"][ok] <= 1), (case, factor, c)
            assert np.isposinf(s["torque_time_scale"][~ok]).all()
            seen.update((s["torque_ratio"][ok] <= 1).tolist())
    assert seen == {True, False}


def test_e_a_restated_trajectory_scales_by_its_factor(made, oracle):
    for case, model, table, dt, J, traj in _gpu_inputs(made, oracle):
        D = model.dof()
        t = dict(table, torque=table["torque"] * 4.0)
        a = tr.truth_torque_score(oracle, model, t, dt, J, traj)
        for c in (1.5, 0.8):
            slow = traj.copy()
            slow[:, :, D:] /= c
            b = tr.truth_torque_score(oracle, model, t, dt * c, J, slow)
            ok = np.isfinite(a["torque_time_scale"])
            assert ok.any()
            assert tr.err(b["torque_time_scale"][ok] * c, a["torque_time_scale"][ok]).max() < 1e-12, (case, c)
            assert tr.err(b["static_ratio"], a["static_ratio"]).max() < 1e-15


def test_f_planted_slips_move_a_torque_of_the_gpu_inputs(made, oracle):
    for case, model, table, dt, J, traj in _gpu_inputs(made, oracle):
        if case[0] not in ("wam", "arm8"):      # one joint has no velocity product, the planar arm's base is not tilted
            continue
        good = tr.reference_torque_score(oracle, model, table, dt, J, traj)["tau"]
        for slip in tr.SLIPS:
            bad = tr.reference_torque_score(oracle, model, table, dt, J, traj, slip)["tau"]
            assert tr.err(bad, good).max() > 100 * tr.CAP, (case, slip)
            assert tr.err(bad, good).max() > 1e-3, (case, slip)      # in fact by far more


def test_the_references_own_error_and_the_undecided_share_on_the_gpu_inputs(made, oracle):
    rows = undecided = 0
    worst = 0.0
    for case, model, table, dt, J, traj in _gpu_inputs(made, oracle):
        ref = tr.reference_torque_score(oracle, model, table, dt, J, traj)
        truth = tr.truth_torque_score(oracle, model, table, dt, J, traj)
        for k in tr.VALUES + ("tau",):
            e = tr.err(ref[k], truth[k]).max()
            worst = max(worst, e)
            assert e <= tr.CAP / 8, (case, k, e)
        assert np.array_equal(ref["invalid"], truth["invalid"]) and (ref["invalid"] == 0).all()
        for c in range(3):
            d = tr.decided(ref, c)
            rows += d.size
            undecided += int((~d).sum())
            same = (ref["worst"][:, c] == truth["worst"][:, c]).all(axis=1)
            assert same[d].all(), (case, c)
    print(f"largest e_cpu {worst:.2e}; undecided {undecided} of {rows}")
    assert undecided * 8 <= rows


@pytest.mark.parametrize("NJ", tr.SHAPES, ids=lambda x: f"N{x[0]}J{x[1]}")
def test_constructed_rows_have_their_known_answers_in_the_reference(made, oracle, NJ):
    N, J = NJ
    model, ro, table = made["wam"]
    dt = tr.case_dt(N)
    rest = np.zeros((1, 2, 14))
    rest[:, :, :7] = tr.REST
    only = np.full(7, np.inf)
    only[tr.PEAK_JOINT] = table["torque"][tr.PEAK_JOINT]
    t_only = dict(table, torque=only)
    sign = np.sign(tr.reference_torque_score(oracle, model, t_only, dt, 0, rest)["tau_g"][0, 0, tr.PEAK_JOINT])
    rows = tr.constructed_rows(N, dt, sign)
    with np.errstate(invalid="ignore"):
        s = tr.reference_torque_score(oracle, model, t_only, dt, J, rows)
    m = tr.PEAK_STATE * (J + 1)
    L = only[tr.PEAK_JOINT]
    assert s["torque_ratio"][0] == s["static_ratio"][0] and s["torque_time_scale"][0] == 0
    for b in (1, 2):
        assert tuple(s["worst"][b, 0]) == (m, tr.PEAK_JOINT) and tuple(s["worst"][b, 2]) == (m, tr.PEAK_JOINT)
    assert s["torque_ratio"][1] == abs(s["tau"][1, m, tr.PEAK_JOINT]) / L            # the right-sided value is the peak
    assert s["torque_ratio"][2] == abs(s["tau_left"][2, m, tr.PEAK_JOINT]) / L       # the left-sided one
    assert s["torque_ratio"][2] > abs(s["tau"][2, m, tr.PEAK_JOINT]) / L
    assert s["invalid"][3] > 0 and (s["invalid"][:3] == 0).all()
    weak = tr.reference_torque_score(oracle, model, dict(table, torque=np.full(7, 0.01)), dt, J, rows[:1])
    assert weak["static_ratio"][0] >= 1 and np.isposinf(weak["torque_time_scale"][0])
