"""The self-collision table of a plan (include/gpmp2mi.h "self-collision table in a plan") as far as the CPU oracle alone
can say: the numpy reference (tests/selfpair_reference.py) equals the oracle's own in-graph self-collision rows where both
exist (P <= 16), the tables of tests/test_gpu_selfpair.py have the hinge branches and the chunk pattern they claim, the
factor moves the scenario's solve, and that solve is well conditioned."""
import copy

import numpy as np
import pytest

import moving_reference as mr
import selfpair_reference as spr
from parity_bound import EPS


def _args(p):
    return p.start_conf, p.start_vel, p.end_conf, p.end_vel


def _handles(oracle, p):
    return oracle.robot(p.model), oracle.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)


@pytest.mark.parametrize("name", ["wam", "config5"])
def test_reference_equals_the_in_graph_rows_of_the_oracle(oracle, name):
    """both are double-precision routes that differ only in the order of their sums"""
    p, traj = mr.plan_case(name)
    N = p.setting.total_step
    ro, so = _handles(oracle, p)
    table = spr.near_table(oracle, p.model, ro, traj, spr.case_ids(name, p.model))[:16]
    assert 2 <= len(table) <= 16 and len(set(table[:, 3])) >= 2
    states = (1, N - 1)
    err, _, _ = spr.rows(oracle, p.model, ro, traj[:, 1:N, :p.setting.dof].reshape(-1, p.setting.dof), table)
    assert (err > 0).any() and (err == 0).any()
    q = copy.deepcopy(p)
    q.setting.self_collision = table
    q.setting.self_collision_states = states
    want = oracle.linearize(ro, so, q.setting, *_args(q), traj)
    got = spr.linearize(oracle, ro, so, p, traj, dict(table=table, states=states))
    plain = oracle.linearize(ro, so, p.setting, *_args(p), traj)
    assert np.abs(want[0] - plain[0]).max() > 0          # the rows are in the oracle's graph
    for x, y in zip(got[:3], want[:3]):
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-12 * np.abs(y).max())
    np.testing.assert_allclose(got[3], want[3], rtol=1e-12)
    np.testing.assert_allclose(spr.graph_error(oracle, ro, so, p, traj, dict(table=table, states=states)),
                               oracle.graph_error(ro, so, q.setting, *_args(q), traj), rtol=1e-12)


@pytest.mark.parametrize("name", mr.PLAN_CASES)
def test_the_gpu_tables_have_both_hinge_branches(oracle, name):
    p, traj = mr.plan_case(name)
    N, D = p.setting.total_step, p.setting.dof
    ro, _ = _handles(oracle, p)
    ids = spr.case_ids(name, p.model)
    table = spr.near_table(oracle, p.model, ro, traj, ids)
    err, H, dist = spr.rows(oracle, p.model, ro, traj[:, 1:N, :D].reshape(-1, D), table)
    print(f"{name}: P = {len(table)}, {int((err > 0).sum())} of {err.size} rows on, smallest distance {dist.min():.3e}")
    assert (err > 0).any() and (err == 0).any() and np.isfinite(H).all() and dist.min() > 0
    assert len(set(table[:, 3])) >= 2 and len(set(table[:, 2])) >= 2
    # no state on the edge of the hinge, in this table and in the second one of the device test
    assert spr.hinge_margin(oracle, p.model, ro, traj, table) > spr.HINGE_MARGIN
    assert spr.hinge_margin(oracle, p.model, ro, traj, spr.near_table(oracle, p.model, ro, traj, ids[::2])) > spr.HINGE_MARGIN
    if name == "pr2":
        assert len(table) > 1000 and p.model.nr_body_spheres() == 65


def test_the_wam_tables_have_the_chunk_pattern_they_claim(oracle):
    p, traj = mr.plan_case("wam")
    N = p.setting.total_step
    ro, _ = _handles(oracle, p)
    ids = spr.case_ids("wam", p.model)
    assert len(ids) >= max(spr.WAM_SIZES)
    table = spr.chunk_table(oracle, p.model, ro, traj, ids)
    assert len(table) >= 130
    on = spr.chunk_activity(oracle, p.model, ro, traj, table, (1, N - 1))
    assert list(on) == [True, False, True]
    # the second chunk is off in every single state, not only as a whole
    err, _, dist = spr.rows(oracle, p.model, ro, traj[:, :, :7].reshape(-1, 7), table)
    assert (err[:, 64:128] == 0).all() and (err[:, :64] > 0).any() and (err[:, 128:] > 0).any()
    assert spr.hinge_margin(oracle, p.model, ro, traj, table) > spr.HINGE_MARGIN
    for P in spr.WAM_SIZES:
        t = spr.near_table(oracle, p.model, ro, traj, spr.varied_pairs(oracle, p.model, ro, traj, ids, P))
        e = spr.rows(oracle, p.model, ro, traj[:, 1:N, :7].reshape(-1, 7), t)[0]
        assert len(t) == P and (e > 0).any() and (e == 0).any() and e.max() > 1e-3
        assert spr.hinge_margin(oracle, p.model, ro, traj, t) > spr.HINGE_MARGIN


def test_the_duplicated_sphere_has_distance_zero_on_the_oracle(oracle):
    model, (a, b) = spr.duplicated_sphere_model()
    ro = oracle.robot(model)
    c, _ = oracle.sphere_centers(ro, np.linspace(-1.0, 1.0, 21).reshape(3, 7))
    assert np.array_equal(c[:, a].view(np.int64), c[:, b].view(np.int64))
    err, H, dist = spr.rows(oracle, model, ro, np.zeros((1, 7)), [[a, b, 0.05, 0.01]])
    te = 2 * model.spheres[a].radius + 0.05
    assert dist[0, 0] == 0.0 and err[0, 0] == te and (H == 0).all()


@pytest.fixture(scope="module")
def scen(oracle):
    p = spr.scenario()
    ro, so = _handles(oracle, p)
    sp = dict(table=spr.wam_table(oracle, p.model, ro), states=(0, p.setting.total_step))
    assert sp["table"].shape == (78, 4)
    return p, ro, so, sp, spr.gauss_newton(oracle, ro, so, p, sp, spr.ITERS)


def test_the_factor_moves_the_scenario(oracle, scen):
    p, ro, so, sp, with_table = scen
    plain = spr.gauss_newton(oracle, ro, so, p, None, spr.ITERS)
    moved = np.abs(with_table - plain).max()
    print(f"the 78-pair table at ({spr.EPSILON}, {spr.SIGMA}) moves the loop by {moved:.3g}")
    assert moved > 1e-2


def test_the_scenario_is_well_conditioned(oracle, scen):
    """the loop's change under a 2-ulp perturbation of the initial values: far below the 1e-6 of the device comparison"""
    p, ro, so, sp, with_table = scen
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(3):
        init = p.init * (1.0 + 2 * EPS * rng.choice([-1.0, 1.0], size=p.init.shape))
        worst = max(worst, np.abs(spr.gauss_newton(oracle, ro, so, p, sp, spr.ITERS, init=init) - with_table).max())
    print(f"2-ulp sensitivity of the loop: {worst:.2e}")
    assert worst < 1e-9
