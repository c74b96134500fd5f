"""Pins the yardstick of tests/backward_error.py on the CPU oracle: the block-row backward error eta of the oracle's own
step stays at a few units of roundoff (<= 1e-14) whatever the trajectory length, and two injected errors of relative
size 1e-10 -- far below what the end-to-end parity gates see -- both push it above 1e-13:

  * the normal equations solved with one coupling block scaled by 1 + 1e-10 (a wrong Schur term),
  * one block of the step scaled by 1 + 1e-10 (a wrong back-substitution), at blocks 0, 1, N / 2 and N.

The GPU cases of tests/test_gpu_step_backward_error.py are admitted below 1e-13 only; this file is what says that such
a bound separates a correct solver from a subtly wrong one."""
import numpy as np
import pytest

from backward_error import eta, eta_block_rows, is_lie, local_coordinates, one_step_setting, step_of
from gpmp2_amd import problems

CLEAN = 1e-14      # the oracle's own step
CAUGHT = 1e-13     # either injected error
REL = 1e-10


def _args(p):
    return p.start_conf, p.start_vel, p.end_conf, p.end_vel


def _oracle_step(oracle, p, opt):
    """(Hd, Ho, g at the initial values, the oracle's first step, lambda) of trajectory 0"""
    st = one_step_setting(p.setting, opt)
    ro, so = oracle.robot(p.model), oracle.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    Hd, Ho, g, _ = oracle.linearize(ro, so, st, *_args(p), p.init)
    dx, res = step_of(oracle, p.init, is_lie(p.model), ro, so, st, *_args(p))
    assert list(res["iters"]) == [1] * p.B
    assert np.abs(dx).max() > 0
    return Hd[0], Ho[0], g[0], dx[0], (st.lm_lambda_initial if opt == "LM" else 0.0)


def _wam(N, prior_sigma=None):
    p = problems.wam_restarts(B=1, total_step=N, obs_check_inter=2, sdf="40")
    if prior_sigma is not None:
        p.setting.set_conf_prior_model(prior_sigma)
        p.setting.set_vel_prior_model(prior_sigma)
    return p


def _cases():
    # N = 1 with the WAM settings has one coupling block between two states that the end-point priors (sigma 1e-4,
    # weight 1e8) hold against a GP block of order 1: scaling that block by 1 + 1e-10 is a backward error of 1e-18 and
    # moves the step by 4e-16 -- not an error any measure should report (measured 1.0e-16).  That case keeps the other
    # two conditions, and N = 1 with end-point priors of sigma 0.1, where the coupling carries weight, takes all three.
    yield pytest.param(lambda: _wam(1), "GN", False, id="wam-N1")
    yield pytest.param(lambda: _wam(1, 0.1), "GN", True, id="wam-N1-loose-priors")
    for N in (9, 33, 100, 300):
        yield pytest.param(lambda N=N: _wam(N), "GN", True, id=f"wam-N{N}")
    yield pytest.param(problems.arm3_planner, "GN", True, id="arm3_planner")
    yield pytest.param(lambda: _wam(17), "LM", True, id="wam-N17-LM-first-step")


@pytest.mark.parametrize("make,opt,coupling", list(_cases()))
def test_oracle_step_is_backward_stable_and_injected_errors_are_not(oracle, make, opt, coupling):
    p = make()
    Hd, Ho, g, dx, lam = _oracle_step(oracle, p, opt)
    nb = g.shape[0]
    clean = eta(Hd, Ho, g, dx, lam)
    print(f"eta of the oracle's step: {clean:.2e}")
    # for LM this also says that the oracle accepted its first trial: against the next rung, 10 lambda_0, the same
    # step is off by ~1e-2
    assert clean <= CLEAN
    if opt == "LM":
        assert eta(Hd, Ho, g, dx, lam * p.setting.lm_lambda_factor) > 1e-4
    # 1. a wrong coupling block (the middle one) in the system that is solved
    bad = Ho.copy()
    bad[(nb - 2) // 2] *= 1.0 + REL
    Hl = Hd + lam * np.eye(Hd.shape[-1])
    x, ok = oracle.block_tridiag_solve(Hl[None], bad[None], -g[None])
    assert ok[0] == 1
    e = eta(Hd, Ho, g, x[0], lam)
    x0, _ = oracle.block_tridiag_solve(Hl[None], Ho[None], -g[None])
    print(f"coupling block scaled: eta {e:.2e}, step moved by {np.abs(x[0] - x0[0]).max():.2e}")
    assert eta(Hd, Ho, g, x0[0], lam) <= CLEAN       # the same solve without the error
    assert e >= CAUGHT or not coupling
    # 2. a wrong block of the step
    for i in sorted({0, 1, nb // 2, nb - 1}):
        y = dx.copy()
        y[i] *= 1.0 + REL
        e = eta(Hd, Ho, g, y, lam)
        print(f"step block {i} scaled: eta {e:.2e}")
        assert e >= CAUGHT, i


def test_a_second_step_can_be_read_back_only_where_the_states_still_move(oracle):
    """Why the update cases of the GPU file loosen the end-point priors: after one step the WAM's priors (sigma 1e-4) hold
    the end states, the second step moves them by ~1e-7, and one rounding of the stored value (1e-16) times the prior's
    weight (1e8) is all there is in those two block rows.  The interior rows, and every row with priors of sigma 0.1, stay
    at roundoff."""
    for sigma, pinned in ((None, True), (0.1, False)):
        p = _wam(9, sigma)
        st = one_step_setting(p.setting, "GN")
        ro, so = oracle.robot(p.model), oracle.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
        first = oracle.batch_optimize(ro, so, st, *_args(p), p.init)["traj"]
        Hd, Ho, g, _ = oracle.linearize(ro, so, st, *_args(p), first)
        dx, _ = step_of(oracle, first, False, ro, so, st, *_args(p))
        rows = eta_block_rows(Hd[0], Ho[0], g[0], dx[0])
        assert rows[1:-1].max() <= CLEAN
        if pinned:
            assert np.abs(dx[0, 0]).max() < 1e-5 and rows[0] > 1e-13
        else:
            assert np.abs(dx[0]).max(axis=1).min() > 1e-3 and rows.max() <= CLEAN


def test_eta_is_zero_for_an_exact_solution_and_sees_each_block_row():
    """Integer data: the residual is exact, so eta is 0 for the solution and names the block row that is off."""
    rng = np.random.default_rng(3)
    nb, n = 5, 3
    Hd = rng.integers(-4, 5, size=(nb, n, n)).astype(float)
    Ho = rng.integers(-4, 5, size=(nb - 1, n, n)).astype(float)
    dx = rng.integers(-4, 5, size=(nb, n)).astype(float)
    H = np.zeros((nb * n, nb * n))
    for i in range(nb):
        H[i * n:(i + 1) * n, i * n:(i + 1) * n] = Hd[i]
        if i + 1 < nb:
            H[(i + 1) * n:(i + 2) * n, i * n:(i + 1) * n] = Ho[i]
            H[i * n:(i + 1) * n, (i + 1) * n:(i + 2) * n] = Ho[i].T
    g = -(H @ dx.reshape(-1)).reshape(nb, n)
    assert eta(Hd, Ho, g, dx) == 0.0
    lam = 2.0
    g2 = g - lam * dx
    assert eta(Hd, Ho, g2, dx, lam) == 0.0 and eta(Hd, Ho, g2, dx) > 0
    g3 = g.copy()
    g3[3, 1] += 1.0
    rows = eta_block_rows(Hd, Ho, g3, dx)
    assert rows[3] > 0 and np.count_nonzero(rows) == 1
    # the denominator of row 3, by hand
    den = sum(np.abs(M).sum(axis=1).max() * np.abs(dx[j]).max()
              for M, j in ((Ho[2], 2), (Hd[3], 3), (Ho[3].T, 4))) + np.abs(g3[3]).max()
    assert float(rows[3]) == pytest.approx(1.0 / den, rel=1e-15)


def test_local_coordinates_invert_the_oracle_retract(oracle):
    """Pose2 robots: the step read back from the values is the step the oracle retracted by."""
    p = problems.mobile_arm_config5()
    ro = oracle.robot(p.model)
    assert is_lie(p.model) and not is_lie(problems.arm3_planner().model)
    rng = np.random.default_rng(8)
    before = p.init[0] + 0.3 * rng.normal(size=p.init[0].shape)
    d = 0.2 * rng.normal(size=before.shape)
    after = oracle.retract(ro, before, d)
    np.testing.assert_allclose(local_coordinates(before, after, True), d, atol=1e-15)
    np.testing.assert_allclose(local_coordinates(before, before + d, False), d, atol=1e-15)
    # a heading step beyond pi comes back modulo 2 pi; a nearby step names the branch
    d[7, 2], d[9, 2] = 3.3, -4.0
    after = oracle.retract(ro, before, d)
    wrapped = local_coordinates(before, after, True)
    np.testing.assert_allclose(wrapped[7, 2] - d[7, 2], -2 * np.pi, atol=1e-14)
    near = d + 0.5 * rng.uniform(-1, 1, size=d.shape)
    np.testing.assert_allclose(local_coordinates(before, after, True, near), d, atol=4e-15)


def test_config5_first_step_turns_the_base_by_more_than_pi(oracle):
    """The Lie case of the GPU file: the oracle's Gauss-Newton step from the initial values of mobile_arm_config5 has
    heading components below -pi, and is backward stable once they are read on the right branch."""
    p = problems.mobile_arm_config5()
    st = one_step_setting(p.setting, "GN")
    ro, so = oracle.robot(p.model), oracle.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    Hd, Ho, g, _ = oracle.linearize(ro, so, st, *_args(p), p.init)
    near, ok = oracle.block_tridiag_solve(Hd, Ho, -g)
    assert ok[0] == 1 and np.abs(near[0, :, 2]).max() > np.pi
    dx, _ = step_of(oracle, p.init, True, ro, so, st, *_args(p), near=near)
    assert eta(Hd[0], Ho[0], g[0], dx[0]) <= CLEAN
    dx_wrapped, _ = step_of(oracle, p.init, True, ro, so, st, *_args(p))
    assert eta(Hd[0], Ho[0], g[0], dx_wrapped[0]) > 1e-6
