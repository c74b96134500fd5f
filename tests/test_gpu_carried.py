"""Carried object on the device (include/gpmp2mi.h "carried object") against the numpy reference on the CPU oracle
(tests/carried_reference.py) and against the augmented robot (the same spheres as body spheres): the factor, the plan's
normal equations and graph error with the factor, whole solves (Gauss-Newton, queue runs, LM, Dogleg), the check of the
executed trajectory with its selection, the argument and state errors that need a live plan, and that plans without
capacity are left alone.

Tolerances are the project's own (tests/test_gpu_moving.py, tests/test_gpu_selfpair.py): rows and normal equations 1e-9
of the largest reference term, errors rtol 1e-9, costs rtol 1e-8 / atol 1e-12, clearances atol 1e-9, final error rtol
1e-8, solved trajectories 1e-6."""
import copy
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import carried_reference as cr
import score_reference as ref
from gpmp2_amd import _capi, problems, scoring
from gpmp2_amd import engine as E

pytestmark = pytest.mark.gpu
FIVE = scoring.CARRIED_NAMES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(p):
    return p.start_conf, p.start_vel, p.end_conf, p.end_vel


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int64) if x.dtype == np.float64 else x


def _same_bits(a, b, rows=None, what="", names=FIVE):
    """the outputs agree bit for bit (rows: (rows of a, rows of b))"""
    for k in names:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows[0]], b[k][rows[1]])
        assert np.array_equal(_bits(x), _bits(y)), (what, k, a[k], b[k])


def _handles(engine, oracle, p):
    return (engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data), oracle.robot(p.model),
            cr.field_of(oracle, p))


# ------------------------------------------------------------------------------------------------ 1. the factor
@pytest.mark.parametrize("A", cr.FACTOR_AS)
@pytest.mark.parametrize("name", list(cr.FACTOR_CASES))
def test_factor_matches_the_reference(engine, oracle, name, A):
    """A below, on and one lane past a chunk of 64; arm3 in a planar field, the WAM in a volume, config5 on the Pose2
    chart in a planar field.  The reference's branches are judged in tests/test_carried_cpu.py."""
    p, traj = cr.plan_case(name)
    D = p.setting.dof
    r, s, ro, field = _handles(engine, oracle, p)
    link0, eps = cr.FACTOR_CASES[name]
    link = cr.link_of(p.model, link0)
    radius, centers = cr.spheres(A, 40 + A)
    conf = np.ascontiguousarray(traj[:, :, :D]).reshape(-1, D)
    err, H = engine.carried_sphere_factor(r, s, link, radius, centers, eps, conf)
    e_ref, H_ref, inr, _ = cr.hinge_rows(oracle, ro, field, conf, link, radius, centers, eps)
    de, dH = np.abs(err - e_ref).max(), np.abs(H - H_ref).max()
    print(f"{name} A={A}: {int((e_ref > 0).sum())} of {e_ref.size} rows active, {int((~inr).sum())} outside the field, "
          f"max |d err| {de:.2e}, max |d H| {dH:.2e}")
    assert err.shape == (conf.shape[0], A) and H.shape == (conf.shape[0], A, D)
    assert ((e_ref > 0) == (err > 0)).all()                             # the same hinge branch everywhere
    assert de <= 1e-9 * max(np.abs(e_ref).max(), 1.0)
    assert dH <= 1e-9 * max(np.abs(H_ref).max(), 1.0)
    assert (err[~inr] == 0.0).all() and (H[~inr] == 0.0).all()          # out of the field: exact zeros
    assert (H[err == 0.0] == 0.0).all()                                 # an inactive row is a zero row
    e_only, none = engine.carried_sphere_factor(r, s, link, radius, centers, eps, conf, jac=False)
    assert none is None and np.array_equal(_bits(e_only), _bits(err))
    # a NaN configuration: every centre fails the range test, nothing is looked up
    bad = conf[:2].copy()
    bad[1] = np.nan
    e_bad, H_bad = engine.carried_sphere_factor(r, s, link, radius, centers, eps, bad)
    assert (e_bad[1] == 0.0).all() and (H_bad[1] == 0.0).all()
    assert np.array_equal(_bits(e_bad[0]), _bits(err[0])) and np.array_equal(_bits(H_bad[0]), _bits(H[0]))


# ------------------------------------------------------------------------------------ 2. linearize and graph error
def _compare_linearize(pl, oracle, ro, field, p, traj, c, label):
    a = pl.linearize(traj)
    b = cr.linearize(oracle, ro, field, p, traj, c)
    worst = [float(np.abs(x - y).max() / np.abs(y).max()) for x, y in zip(a[:3], b[:3])]
    rel = float(np.abs(a[3] / b[3] - 1.0).max())
    ge = pl.graph_error(traj)
    print(f"{label}: max |d Hd|, |d Ho|, |d g| over max|ref| {worst}, error rel {rel:.2e}, "
          f"graph_error rel {float(np.abs(ge / b[3] - 1.0).max()):.2e}")
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-9 * np.abs(y).max(), err_msg=label)
    np.testing.assert_allclose(a[3], b[3], rtol=1e-9, err_msg=label)
    np.testing.assert_allclose(ge, b[3], rtol=1e-9, err_msg=label)
    return a, b


@pytest.mark.parametrize("name", cr.PLAN_CASES)
def test_plan_linearize_and_graph_error_carry_the_factor(engine, oracle, name):
    """B = 3, states (1, N - 1), capacity 200: narrow (arm3, WAM, config5: Pose2 chart), wide (mobile WAM, dof 10) and
    dense (PR2) blocks.  A = 0 is oracle.linearize alone; two sets in a row on two different links (A = 65, then A = 3)
    are both reflected without recreating the plan; a 192-sphere set whose middle chunk is inactive takes the ballot
    skip."""
    p, traj = cr.plan_case(name)
    N, D = p.setting.total_step, p.setting.dof
    link0, eps = cr.PLAN_SETS[name]
    states = (1, N - 1)
    p.setting.set_carried_spheres(200, eps, cr.SIGMA, states=states)
    r, s, ro, field = _handles(engine, oracle, p)
    pl = engine.plan(r, s, p.setting, p.B)
    pl.set_problem(*_args(p), p.init)
    assert pl.carried_count() == 0
    base, _ = _compare_linearize(pl, oracle, ro, field, p, traj, None, f"{name} A=0")
    first = cr.link_of(p.model, link0)
    sets = [(first, *cr.spheres(65, 105)), (cr.SECOND_LINK[name], *cr.spheres(3, 106, far=False)),
            (first, *cr.middle_inactive_set(oracle, ro, field, p, traj, first, eps, states))]
    for k, (link, radius, centers) in enumerate(sets):
        c = dict(link=link, radius=radius, centers=centers, epsilon=eps, sigma=cr.SIGMA, states=states)
        pl.set_carried(link, radius, centers)
        A = len(radius)
        assert pl.carried_count() == A
        G, gg, e = cr.plan_terms(oracle, ro, field, D, traj, c)
        if k != 1:
            assert (e > 0).any() and np.abs(G).max() > 0          # the factor is on
        got, want = _compare_linearize(pl, oracle, ro, field, p, traj, c, f"{name} link {link} A={A}")
        for x, y in zip(got, pl.linearize(traj)):
            assert np.array_equal(_bits(x), _bits(y))             # the same bits on a second run
        # states outside the range are untouched: their blocks are those of the plan with the empty set
        for i in (0, N):
            assert np.array_equal(_bits(got[0][:, i]), _bits(base[0][:, i])), i
            assert np.array_equal(_bits(got[2][:, i]), _bits(base[2][:, i])), i
        # The factor's own share, free of the 1e8 priors of states 0 and N that set the scale of the bound above: what
        # the spheres add to the blocks of states 1 .. N - 1 against the reference terms.  Bound: the project's 1e-9 of
        # the terms, plus the cancellation of the subtraction (a few ulp of the interior blocks).
        inner = slice(1, N)
        ulp = 8 * np.finfo(np.float64).eps
        dG = np.abs((got[0] - base[0])[:, inner, :D, :D] - G[:, inner]).max()
        dg = np.abs((got[2] - base[2])[:, inner, :D] - gg[:, inner]).max()
        de = np.abs((got[3] - base[3]) - e).max()
        print(f"{name} link {link} A={A}: the factor's share: |d G| {dG:.2e} of {np.abs(G).max():.2e}, |d g| {dg:.2e} of "
              f"{np.abs(gg).max():.2e}, |d e| {de:.2e} of {e.max():.2e}")
        assert dG <= 1e-9 * np.abs(G).max() + ulp * np.abs(base[0][:, inner]).max()
        assert dg <= 1e-9 * np.abs(gg).max() + ulp * np.abs(base[2][:, inner]).max()
        assert de <= 1e-9 * e.max() + ulp * base[3].max()
        assert np.array_equal((got[0] - base[0])[:, :, D:, :], np.zeros_like(got[0][:, :, D:, :]))   # velocities: nothing
    pl.set_carried(0, None, None)
    for x, y in zip(base, pl.linearize(traj)):
        assert np.array_equal(_bits(x), _bits(y))                 # cleared: the plan with the empty set
    pl.close()


# -------------------------------------------------------------------------------- 3. the augmented-robot identity
@pytest.fixture(scope="module")
def scen(engine, oracle):
    p, c = cr.scenario()
    r, s, ro, field = _handles(engine, oracle, p)
    return dict(p=p, c=c, r=r, s=s, ro=ro, field=field)


def _scenario_plan(engine, sc, p, B=None):
    q = copy.deepcopy(p)
    c = sc["c"]
    q.setting.set_carried_spheres(len(c["radius"]), c["epsilon"], c["sigma"])
    pl = engine.plan(sc["r"], sc["s"], q.setting, B or q.B)
    pl.set_carried(c["link"], c["radius"], c["centers"])
    return q, pl


def test_the_plan_is_the_augmented_robot(engine, oracle, scen):
    """I = 0, the factor on all states with the setting's epsilon and sigma: linearize is the oracle's linearization of
    the robot with the spheres appended as body spheres; a fixed-iteration GN solve is the reference loop; after
    set_carried(A = 0) the same plan solves the plain problem."""
    sc = scen
    p, c = copy.deepcopy(sc["p"]), sc["c"]
    p.setting.fixed_iterations = cr.ITERS
    q, pl = _scenario_plan(engine, sc, p)
    pl.set_problem(*_args(q), q.init)
    ra = oracle.robot(cr.augmented(p.model, c["link"], c["radius"], c["centers"]))
    a = pl.linearize(q.init)
    b = oracle.linearize(ra, sc["field"].handle, p.setting, *_args(p), p.init)
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-9 * np.abs(y).max())
    np.testing.assert_allclose(a[3], b[3], rtol=1e-9)
    pl.optimize()
    res = pl.result()
    want = cr.gauss_newton(oracle, sc["ro"], sc["field"], p, c, cr.ITERS)
    plain = cr.gauss_newton(oracle, sc["ro"], sc["field"], p, None, cr.ITERS)
    d = np.abs(res["traj"] - want).max()
    print(f"GN x{cr.ITERS}: max |traj - reference| {d:.2e}; the object moves the reference by {np.abs(want - plain).max():.2e}")
    assert list(res["iters"]) == [cr.ITERS] * p.B
    assert d <= 1e-6 and np.abs(want - plain).max() > 1e-2
    e_ref = cr.graph_error(oracle, sc["ro"], sc["field"], p, res["traj"], c)
    np.testing.assert_allclose(res["final_error"], e_ref, rtol=1e-8)
    pl.set_carried(c["link"], None, None)
    pl.set_problem(*_args(q), q.init)
    pl.optimize()
    assert np.abs(pl.result()["traj"] - plain).max() <= 1e-6
    pl.close()


@pytest.mark.parametrize("opt", ["LM", "DOGLEG"])
def test_lm_and_dogleg_report_the_error_with_the_factor(engine, oracle, scen, opt):
    sc = scen
    p, c = copy.deepcopy(sc["p"]), sc["c"]
    {"LM": p.setting.setLM, "DOGLEG": p.setting.setDogleg}[opt]()
    q, pl = _scenario_plan(engine, sc, p)
    pl.set_problem(*_args(q), q.init)
    pl.optimize()
    res = pl.result()
    e_ref = cr.graph_error(oracle, sc["ro"], sc["field"], p, res["traj"], c)
    e_plain = oracle.graph_error(sc["ro"], sc["field"].handle, p.setting, *_args(p), res["traj"])
    print(f"{opt}: iters {res['iters']}, final_error {res['final_error']}, rel to the reference "
          f"{np.abs(res['final_error'] / e_ref - 1).max():.2e}; the factor's share {e_ref - e_plain}")
    np.testing.assert_allclose(res["final_error"], e_ref, rtol=1e-8)
    assert (res["iters"] >= 1).all()
    for b in range(p.B):
        tr = res["error_trace"][b]
        tr = tr[~np.isnan(tr)]
        assert tr.size >= 1 and (np.diff(tr) <= 0).all() and res["final_error"][b] <= tr[0], (b, tr)
    pl.close()


# -------------------------------------------------------------------------------------------------- 4. queue run
def test_queue_run_with_slot_refill_equals_the_reference_loop(engine, oracle, scen):
    """M = 5 problems through B = 3 slots"""
    sc = scen
    p5 = problems.wam_restarts(B=5, total_step=10, obs_check_inter=0, sdf="40")
    p5.setting.fixed_iterations = cr.ITERS
    q, pl = _scenario_plan(engine, sc, p5, B=3)
    res = pl.optimize_queue(*_args(q), q.init)
    want = cr.gauss_newton(oracle, sc["ro"], sc["field"], p5, sc["c"], cr.ITERS)
    d = np.abs(res["traj"] - want).reshape(5, -1).max(axis=1)
    print(f"queue 5 through 3: max |traj - reference| per problem {d}")
    assert list(res["iters"]) == [cr.ITERS] * 5
    assert d.max() <= 1e-6
    pl.close()


# ---------------------------------------------------------------------------------------------------- 5. the check
def _check_against_reference(dev, exp, label):
    B = len(exp["out_of_range"])
    finite = np.isfinite(exp["min_carried_clearance"])
    dclr = np.abs(dev["min_carried_clearance"][finite] - exp["min_carried_clearance"][finite]).max() if finite.any() else 0.0
    print(f"{label}: max |d support| {np.abs(dev['carried_support_cost'] - exp['carried_support_cost']).max():.2e}, "
          f"max |d dense| {np.abs(dev['carried_dense_cost'] - exp['carried_dense_cost']).max():.2e}, "
          f"max |d clearance| {dclr:.2e}, gaps {exp['gap']}")
    np.testing.assert_allclose(dev["carried_support_cost"], exp["carried_support_cost"], rtol=1e-8, atol=1e-12, err_msg=label)
    np.testing.assert_allclose(dev["carried_dense_cost"], exp["carried_dense_cost"], rtol=1e-8, atol=1e-12, err_msg=label)
    np.testing.assert_allclose(dev["min_carried_clearance"], exp["min_carried_clearance"], rtol=0, atol=1e-9, err_msg=label)
    assert np.array_equal(dev["out_of_range"], exp["out_of_range"]), (label, dev["out_of_range"], exp["out_of_range"])
    # worst: the reference's argmin wherever its runner-up is more than 1e-6 above the minimum; a closer row whose
    # pair differs is excused, at most 10 % of the rows (tests/test_carried_cpu.py: the inputs keep to that)
    with np.errstate(invalid="ignore"):
        decided = ~(exp["gap"] <= 1e-6)
    differs = (dev["worst"] != exp["worst"]).any(axis=1)
    assert not (differs & decided).any(), (label, dev["worst"][differs], exp["worst"][differs], exp["gap"][differs])
    assert differs.sum() <= 0.1 * B, (label, "rows excused", int(differs.sum()), B)


@pytest.mark.parametrize("name,J", cr.CHECK_CASES, ids=[f"{n}-J{j}" for n, j in cr.CHECK_CASES])
def test_check_matches_the_reference(engine, oracle, name, J):
    p, traj = cr.plan_case(name)
    r, s, ro, field = _handles(engine, oracle, p)
    link = cr.link_of(p.model, cr.PLAN_SETS[name][0])
    radius, centers = cr.spheres(65, 105)
    dt = ref.delta_t(p.setting)
    exp = cr.oracle_carried_score(oracle, p.model, ro, field, link, radius, centers, dt, J, traj)
    dev = engine.carried_score_traj(r, s, link, radius, centers, dt, J, traj)
    _check_against_reference(dev, exp, f"{name} J={J}")
    if J == 0:   # the support states are all there is: the two sums are the same additions
        assert np.array_equal(_bits(dev["carried_dense_cost"]), _bits(dev["carried_support_cost"]))
    assert (dev["carried_dense_cost"] > 0).any() and (dev["min_carried_clearance"] < 0).any()
    # a row alone, and in another batch at another position: the same bits
    alone = engine.carried_score_traj(r, s, link, radius, centers, dt, J, traj[1])
    _same_bits(alone, dev, rows=(0, 1), what="alone vs row 1 of 3")
    other = np.concatenate([traj[2:], traj[:1], traj[1:2], traj[:2]])
    _same_bits(engine.carried_score_traj(r, s, link, radius, centers, dt, J, other), dev, rows=(2, 1),
               what="row 2 of 5 vs row 1 of 3")
    # an empty set: +inf, (-1, -1), nothing out of range
    none = engine.carried_score_traj(r, s, link, None, None, dt, J, traj)
    assert (none["carried_dense_cost"] == 0.0).all() and np.isposinf(none["min_carried_clearance"]).all()
    assert (none["worst"] == -1).all() and (none["out_of_range"] == 0).all()
    # a NaN row is out of range everywhere and leaves its neighbours' bits alone
    bad = traj.copy()
    bad[1] = np.nan
    sc = engine.carried_score_traj(r, s, link, radius, centers, dt, J, bad)
    Md = scoring.checked_states(p.setting.total_step, J)
    assert sc["out_of_range"][1] == Md * 65
    assert sc["carried_dense_cost"][1] == 0.0 and sc["carried_support_cost"][1] == 0.0
    assert np.isposinf(sc["min_carried_clearance"][1]) and tuple(sc["worst"][1]) == (-1, -1)
    _same_bits(sc, dev, rows=([0, 2], [0, 2]), what="ordinary rows beside a NaN row")


@pytest.fixture(scope="module")
def solved(engine, oracle, scen):
    """the scenario solved on the device WITHOUT the object (an empty set), then given it: rows that touch obstacles"""
    sc = scen
    p = copy.deepcopy(sc["p"])
    p.setting.fixed_iterations = cr.ITERS
    q = copy.deepcopy(p)
    q.setting.set_carried_spheres(16, sc["c"]["epsilon"], sc["c"]["sigma"])
    pl = engine.plan(sc["r"], sc["s"], q.setting, q.B)
    pl.set_problem(*_args(q), q.init)
    pl.optimize()
    res = pl.result()
    pl.set_carried(sc["c"]["link"], sc["c"]["radius"], sc["c"]["centers"])
    return dict(sc, pl=pl, res=res, q=q, dt=ref.delta_t(q.setting))


def test_the_plan_form_scores_the_same_bits_as_the_trajectory_form(engine, oracle, solved):
    w = solved
    pl, c, traj = w["pl"], w["c"], w["res"]["traj"]
    for J in (0, 4):
        through_plan = pl.carried_score(J)
        exp = cr.oracle_carried_score(oracle, w["p"].model, w["ro"], w["field"], c["link"], c["radius"], c["centers"], w["dt"], J, traj)
        _check_against_reference(through_plan, exp, f"scenario through the plan, J={J}")
        batch = engine.carried_score_traj(w["r"], w["s"], c["link"], c["radius"], c["centers"], w["dt"], J, traj)
        _same_bits(through_plan, batch, what="Plan.carried_score vs Engine.carried_score_traj on the fetched result")
        _same_bits(through_plan, pl.carried_score(J), what="Plan.carried_score twice in a row")
    part = pl.carried_score(4, out={"min_carried_clearance": np.zeros(3)})
    assert np.array_equal(_bits(part["min_carried_clearance"]), _bits(through_plan["min_carried_clearance"]))


# ------------------------------------------------------------------------------------------------- 6. the selection
def test_select_carried_is_the_extended_rule_on_the_reference_scores(engine, oracle, solved):
    w = solved
    pl, c, res, J = w["pl"], w["c"], w["res"], 4
    p = w["p"]
    ob = ref.oracle_score(oracle, p.model, w["ro"], w["field"], w["dt"], J, res["traj"])
    co = cr.oracle_carried_score(oracle, p.model, w["ro"], w["field"], c["link"], c["radius"], c["centers"], w["dt"], J, res["traj"])
    plain = pl.select(J, -np.inf, False)
    b0 = plain["best"]
    assert b0 >= 0 and plain["n_eligible"] == 3
    clr = co["min_carried_clearance"]
    thr = clr[b0] + 1e-3            # a threshold that the best row by error fails
    assert (np.abs(clr - thr) > 1e-6).all()
    want = scoring.carried_rule(res["final_error"], res["status"], ob["min_clearance"], ob["out_of_range"], -np.inf, False,
                                min_carried_clearance=clr, carried_out_of_range=co["out_of_range"],
                                required_carried_clearance=thr)
    got = pl.select_carried(J, thr, required_clearance=-np.inf)
    print(f"select {b0} of {plain['n_eligible']}; carried clearances {clr}; select_carried(>= {thr:.4f}) {got['best']} of "
          f"{got['n_eligible']}, reference {want}")
    assert (got["best"], got["n_eligible"]) == want and want[0] != b0
    if want[0] >= 0:
        assert np.array_equal(_bits(got["traj_best"]), _bits(res["traj"][want[0]]))
    pairs = engine.generate_self_pairs(w["r"], 2, np.zeros((1, 7)))
    import self_reference as sr
    se = sr.oracle_self_score(oracle, p.model, w["ro"], pairs.data, w["dt"], J, res["traj"])
    for req, rir, req_self, req_c, with_pairs in ((0.0, True, 0.0, -np.inf, False), (-np.inf, False, -np.inf, -0.25, True),
                                                  (-np.inf, False, 0.0, float(np.sort(clr)[1]) - 1e-3, True),
                                                  (-np.inf, True, 0.0, -np.inf, False), (0.0, False, 0.0, 10.0, False)):
        a = pl.select_carried(J, req_c, required_clearance=req, require_in_range=rir,
                              pairs=pairs if with_pairs else None, required_self_clearance=req_self)
        b = scoring.carried_rule(res["final_error"], res["status"], ob["min_clearance"], ob["out_of_range"], req, rir,
                                 se["min_self_clearance"] if with_pairs else None, se["invalid"] if with_pairs else None,
                                 req_self, clr, co["out_of_range"], req_c)
        assert (a["best"], a["n_eligible"]) == b, (req, rir, req_self, req_c, with_pairs, a["best"], a["n_eligible"], b)
    none = pl.select_carried(J, 10.0, required_clearance=-np.inf)
    assert (none["best"], none["n_eligible"]) == (-1, 0) and none["traj_best"] is None and none["dense_best"] is None
    # the empty set and -inf: the row of the existing calls
    pl.set_carried(c["link"], None, None)
    for req, rir in ((-np.inf, False), (0.0, True)):
        a, b = pl.select_carried(J, -np.inf, required_clearance=req, require_in_range=rir), pl.select(J, req, rir)
        assert (a["best"], a["n_eligible"]) == (b["best"], b["n_eligible"])
        if b["best"] >= 0:
            assert np.array_equal(_bits(a["dense_best"]), _bits(b["dense_best"]))
    a = pl.select_carried(J, -np.inf, required_clearance=-np.inf, pairs=pairs, required_self_clearance=-np.inf)
    b = pl.select_checked(J, pairs, -np.inf, False, -np.inf)
    assert (a["best"], a["n_eligible"]) == (b["best"], b["n_eligible"])
    empty = pl.carried_score(J)
    assert np.isposinf(empty["min_carried_clearance"]).all() and (empty["worst"] == -1).all()
    pl.set_carried(c["link"], c["radius"], c["centers"])
    pairs.close()


_DEV = r"""
import copy
import numpy as np
import torch                      # torch's HIP runtime first, as bench.py does
torch.cuda.init()
import carried_reference as cr
import score_reference as ref
from gpmp2_amd import engine as E
eng = E.Engine()
p, c = cr.scenario()
p.setting.fixed_iterations = cr.ITERS
q = copy.deepcopy(p)
q.setting.set_carried_spheres(16, c["epsilon"], c["sigma"])
r, s = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
pl = eng.plan(r, s, q.setting, q.B)
pl.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
pl.optimize()
res = pl.result()
J, B, N, D, A = 4, q.B, q.setting.total_step, q.setting.dof, len(c["radius"])
Md = N * (J + 1) + 1
pl.set_carried(c["link"], c["radius"], c["centers"])
lin_host = pl.linearize(p.init)
host = pl.carried_score(J)
thr = float(np.sort(host["min_carried_clearance"])[1]) - 1e-3
want = pl.select_carried(J, thr, required_clearance=-np.inf)
dev = torch.device("cuda:0")
f = lambda shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
i = lambda shape: torch.full(shape, -7, dtype=torch.int32, device=dev)
rad, cen = torch.from_numpy(c["radius"]).to(dev), torch.from_numpy(c["centers"]).to(dev)
traj = torch.from_numpy(res["traj"]).to(dev)
torch.cuda.synchronize()
st = torch.cuda.Stream(device=dev)
pl.set_carried(c["link"], None, None)
outs = dict(carried_support_cost=f((B,)), carried_dense_cost=f((B,)), min_carried_clearance=f((B,)), worst=i((B, 2)),
            out_of_range=i((B,)))
outs2 = {k: v.clone() for k, v in outs.items()}
best, n, tb, db = i((1,)), i((1,)), f((N + 1, 2 * D)), f((Md, 2 * D))
with torch.cuda.stream(st):
    pl.set_carried_dev(c["link"], A, rad, cen, stream=st.cuda_stream)
    pl.carried_score_dev(J, stream=st.cuda_stream, **outs)
    pl.select_carried_dev(J, thr, required_clearance=-np.inf, best=best, n_eligible=n, traj_best=tb, dense_best=db,
                          stream=st.cuda_stream)
    eng.carried_score_traj_dev(r, s, c["link"], A, rad, cen, ref.delta_t(q.setting), J, B, N, traj, stream=st.cuda_stream,
                               **outs2)
st.synchronize()
assert pl.carried_count() == A
for k in host:
    for o in (outs, outs2):
        got = o[k].cpu().numpy()
        assert np.array_equal(got.view(np.int64) if got.dtype == np.float64 else got,
                              host[k].view(np.int64) if host[k].dtype == np.float64 else host[k]), k
assert (int(best.cpu()[0]), int(n.cpu()[0])) == (want["best"], want["n_eligible"]) and want["best"] >= 0
assert np.array_equal(tb.cpu().numpy().view(np.int64), want["traj_best"].view(np.int64))
assert np.array_equal(db.cpu().numpy().view(np.int64), want["dense_best"].view(np.int64))
for x, y in zip(lin_host, pl.linearize(p.init)):      # the set given through device buffers: the same factor
    assert np.array_equal(x.view(np.int64), y.view(np.int64))
pl.close()
print("CARRIED DEV OK")
"""


def test_dev_forms_equal_the_host_forms_next_to_torch():
    """fresh process: torch initialises the HIP runtime before the library, as bench.py does; the set, the scores and
    the selection through torch device buffers on a torch stream are the host forms' bits"""
    assert importlib.util.find_spec("torch") is not None    # not imported here: this process keeps the library's runtime
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] +
                                                      [x for x in [os.environ.get("PYTHONPATH")] if x]))
    r = subprocess.run([sys.executable, "-c", _DEV], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0 and "CARRIED DEV OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------ 7. errors on a live plan
def test_errors_that_need_a_live_plan(engine, scen):
    sc = scen
    p, c = sc["p"], sc["c"]
    lib = engine.lib
    q, pl = _scenario_plan(engine, sc, p)       # capacity 12, the scenario's set resident
    N, L, A = p.setting.total_step, cr.nr_links(p.model), len(c["radius"])
    for call in (lambda: pl.carried_score(1), lambda: pl.select_carried(1)):     # nothing to score yet
        with pytest.raises(E.Gpmp2miError) as ei:
            call()
        assert ei.value.code == 1 and "not been optimized" in str(ei.value)
    pl.set_problem(*_args(q), q.init)
    before = pl.linearize(q.init)
    # refused calls change nothing: over the capacity, a link out of range, a non-finite centre, a negative / NaN radius
    more_r, more_c = cr.spheres(A + 1, 9, far=False)
    bad_c = c["centers"].copy()
    bad_c[1, 2] = np.inf
    neg, nan = c["radius"].copy(), c["radius"].copy()
    neg[0], nan[1] = -0.01, np.nan
    for link, radius, centers in ((c["link"], more_r, more_c), (L, c["radius"], c["centers"]), (-1, c["radius"], c["centers"]),
                                  (c["link"], c["radius"], bad_c), (c["link"], neg, c["centers"]), (c["link"], nan, c["centers"])):
        with pytest.raises(E.Gpmp2miError) as ei:
            pl.set_carried(link, radius, centers)
        assert ei.value.code == 1
    assert pl.carried_count() == A
    after = pl.linearize(q.init)
    for x, y in zip(before, after):
        assert np.array_equal(_bits(x), _bits(y))                 # the old set is still in force
    assert lib.gpmp2mi_plan_set_carried(pl.h.ptr, c["link"], 1, None, E.dptr(c["centers"])) == 1
    assert lib.gpmp2mi_plan_set_carried(pl.h.ptr, c["link"], -1, E.dptr(c["radius"]), E.dptr(c["centers"])) == 1
    pl.optimize()
    assert lib.gpmp2mi_plan_carried_score(pl.h.ptr, -1, None, None, None, None, None) == 1
    assert lib.gpmp2mi_plan_carried_score(pl.h.ptr, 1, None, None, None, None, None) == 0      # every output may be NULL
    pl.close()
    # the forms without a plan: the link, the values
    conf = np.ascontiguousarray(p.init[0, :2, :p.setting.dof])
    for link, radius, centers in ((L, c["radius"], c["centers"]), (c["link"], neg, c["centers"]), (c["link"], c["radius"], bad_c)):
        with pytest.raises(E.Gpmp2miError) as ei:
            engine.carried_sphere_factor(sc["r"], sc["s"], link, radius, centers, 0.1, conf)
        assert ei.value.code == 1
        with pytest.raises(E.Gpmp2miError) as ei:
            engine.carried_score_traj(sc["r"], sc["s"], link, radius, centers, 0.5, 1, p.init)
        assert ei.value.code == 1
    # a plan created without capacity: an empty set is all it takes, and it has no check
    pl0 = engine.plan(sc["r"], sc["s"], p.setting, p.B)
    pl0.set_problem(*_args(p), p.init)
    pl0.optimize()
    pl0.set_carried(0, None, None)
    with pytest.raises(E.Gpmp2miError) as ei:
        pl0.set_carried(c["link"], c["radius"][:1], c["centers"][:1])
    assert ei.value.code == 1
    for call in (lambda: pl0.carried_score(1), lambda: pl0.select_carried(1)):
        with pytest.raises(E.Gpmp2miError) as ei:
            call()
        assert ei.value.code == 1 and "without room" in str(ei.value)
    pl0.close()
    # creation: the fields are validated before anything is allocated
    for cap, eps, sigma, states in ((257, 0.2, 0.01, None), (-1, 0.2, 0.01, None), (2, 0.2, 0.0, None), (2, 0.2, np.nan, None),
                                    (2, np.inf, 0.01, None), (2, 0.2, 0.01, (3, 2)), (2, 0.2, 0.01, (0, N + 1)),
                                    (2, 0.2, 0.01, (-1, 2))):
        st, o, keep = _capi.make_settings(p.setting)
        o.max_carried_spheres, o.carried_epsilon, o.carried_sigma = cap, eps, sigma
        o.carried_first, o.carried_last = states or (0, N)
        out = C.c_void_p()
        assert lib.gpmp2mi_plan_create(sc["r"].ptr, sc["s"].ptr, C.byref(st), C.byref(o), p.B, C.byref(out)) == 1, (cap, eps, sigma, states)
        assert out.value is None


def _plan_with_opts(engine, r, s, setting, B, edit):
    """a Plan whose gpmp2mi_graph_opts is edit(opts) (None: NULL, the library's defaults)"""
    pl = E.Plan.__new__(E.Plan)
    pl.eng, pl.robot, pl.sdf, pl.setting, pl.B = engine, r, s, setting, int(B)
    st, o, keep = _capi.make_settings(setting)
    o = edit(o)
    pl._keep = (st, o, keep)
    out = C.c_void_p()
    engine._ck(engine.lib.gpmp2mi_plan_create(r.ptr, s.ptr, C.byref(st), None if o is None else C.byref(o), pl.B, C.byref(out)))
    pl.h = E._Handle(out, engine.lib.gpmp2mi_plan_destroy)
    pl.D, pl.N = setting.dof, setting.total_step
    return pl


def _junk_without_capacity(o):
    o.max_carried_spheres = 0
    o.carried_first, o.carried_last, o.carried_epsilon, o.carried_sigma = 7, 3, np.nan, -1.0     # not read without capacity
    return o


def test_plans_without_capacity_are_left_alone(engine):
    """junk in the four other fields is not read, and the linearize bits and the solve equal those of a plan made with
    the default options"""
    p = problems.wam_restarts(B=3, total_step=10, obs_check_inter=2, sdf="40")
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    results = []
    for edit in (lambda o: None, _junk_without_capacity):
        pl = _plan_with_opts(engine, r, s, p.setting, p.B, edit)
        pl.set_problem(*_args(p), p.init)
        lin = pl.linearize(p.init)
        pl.optimize()
        results.append((lin, pl.result()))
        pl.close()
    assert (results[0][1]["iters"] >= 1).all()
    for x, y in zip(results[0][0], results[1][0]):
        assert np.array_equal(_bits(x), _bits(y))
    for k in ("traj", "final_error", "iters", "status"):
        assert np.array_equal(results[0][1][k], results[1][1][k]), k
