"""The self-collision table of a plan on the device (include/gpmp2mi.h "self-collision table in a plan") against the
numpy reference on the CPU oracle (tests/selfpair_reference.py): the plan's normal equations and graph error with the
factor, the dist == 0 rule, P <= 16 through both routes, whole solves with more than 16 pairs (Gauss-Newton, queue runs,
LM, Dogleg), what the feature is for, the errors that need a live plan, and that plans without capacity are left alone.

Tolerances are the project's own, as tests/test_gpu_moving.py states them: normal equations atol 1e-9 max|ref|, errors
rtol 1e-9, final error rtol 1e-8, solved trajectories 1e-6."""
import copy
import ctypes as C

import numpy as np
import pytest

import moving_reference as mr
import parity_bound as pb
import score_reference as ref
import self_reference as sr
import selfpair_reference as spr
from gpmp2_amd import _capi, problems, scoring
from gpmp2_amd import engine as E

pytestmark = pytest.mark.gpu
ULP = 8 * np.finfo(np.float64).eps


def _args(p):
    return p.start_conf, p.start_vel, p.end_conf, p.end_vel


def _handles(engine, oracle, p):
    return (engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data),
            oracle.robot(p.model), oracle.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data))


def _bits(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.int64), np.ascontiguousarray(y).view(np.int64))


def _plan(engine, r, s, p, capacity, states=None, B=None):
    q = copy.deepcopy(p)
    q.setting.set_self_pairs(capacity, states)
    return q, engine.plan(r, s, q.setting, B or q.B)


# ------------------------------------------------------------------------------------ 1. linearize and graph error
def _compare(got, ge, want, label):
    worst = [float(np.abs(x - y).max() / np.abs(y).max()) for x, y in zip(got[:3], want[:3])]
    print(f"{label}: max |d Hd|, |d Ho|, |d g| over max|ref| {worst}, error rel "
          f"{float(np.abs(got[3] / want[3] - 1.0).max()):.2e}, graph_error rel {float(np.abs(ge / want[3] - 1.0).max()):.2e}")
    for x, y in zip(got[:3], want[:3]):
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-9 * np.abs(y).max(), err_msg=label)
    np.testing.assert_allclose(got[3], want[3], rtol=1e-9, err_msg=label)
    np.testing.assert_allclose(ge, want[3], rtol=1e-9, err_msg=label)


def _tables(name, oracle, model, ro, traj):
    ids = spr.case_ids(name, model)
    if name == "wam":
        out = [(f"P={P}", spr.near_table(oracle, model, ro, traj, spr.varied_pairs(oracle, model, ro, traj, ids, P)))
               for P in spr.WAM_SIZES]
        return out + [("chunks on-off-on", spr.chunk_table(oracle, model, ro, traj, ids))]
    return [("full", spr.near_table(oracle, model, ro, traj, ids)), ("every other", spr.near_table(oracle, model, ro, traj, ids[::2]))]


@pytest.mark.parametrize("name", mr.PLAN_CASES)
def test_plan_linearize_and_graph_error_carry_the_factor(engine, oracle, name):
    """B = 3, states (1, N - 1): narrow (arm3, WAM, config5: Pose2 chart), wide (mobile WAM, dof 10) and dense (PR2: 65
    spheres, more than 1 000 pairs, NE = 190) blocks.  The tables follow each other in one plan: a replaced table and a
    cleared one are reflected without recreating it."""
    p, traj = mr.plan_case(name)
    N, D = p.setting.total_step, p.setting.dof
    r, s, ro, so = _handles(engine, oracle, p)
    tables = _tables(name, oracle, p.model, ro, traj)
    states = (1, N - 1)
    q, pl = _plan(engine, r, s, p, max(len(t) for _, t in tables), states)
    pl.set_problem(*_args(p), p.init)
    assert pl.self_pairs_count() == 0
    base = pl.linearize(traj)
    _compare(base, pl.graph_error(traj), spr.linearize(oracle, ro, so, p, traj, None), f"{name} empty")
    inner = slice(1, N)
    if name == "pr2":
        assert len(tables[0][1]) > 16 * 64                       # the generated list: more than 16 chunks
    for label, table in tables:
        h =engine.self_pairs(r, table)
        pl.set_self_pairs(h)
        assert pl.self_pairs_count() == len(table)
        sp = dict(table=table, states=states)
        G, gg, e = spr.plan_terms(oracle, p.model, ro, traj, table, states)
        assert e.max() > 0 and np.abs(G).max() > 0
        got = pl.linearize(traj)
        _compare(got, pl.graph_error(traj), spr.linearize(oracle, ro, so, p, traj, sp), f"{name} {label}")
        for x, y in zip(got, pl.linearize(traj)):
            assert _bits(x, y)                                   # the same bits on a second run
        for i in (0, N):                                         # states outside the range keep the plain plan's bits
            assert _bits(got[0][:, i], base[0][:, i]) and _bits(got[2][:, i], base[2][:, i]), i
        assert _bits(got[1], base[1])                            # the couplings get nothing
        # the factor's own share on the interior states against the reference terms: 1e-9 of the terms plus the
        # cancellation of the subtraction (a few ulp of the interior blocks)
        dG = np.abs((got[0] - base[0])[:, inner, :D, :D] - G[:, inner]).max()
        dg = np.abs((got[2] - base[2])[:, inner, :D] - gg[:, inner]).max()
        de = np.abs((got[3] - base[3]) - e).max()
        print(f"{name} {label}: P = {len(table)}; the factor's share: |d G| {dG:.2e} of {np.abs(G).max():.2e}, |d g| "
              f"{dg:.2e} of {np.abs(gg).max():.2e}, |d e| {de:.2e} of {e.max():.2e}")
        assert dG <= 1e-9 * np.abs(G).max() + ULP * np.abs(base[0][:, inner]).max()
        assert dg <= 1e-9 * np.abs(gg).max() + ULP * np.abs(base[2][:, inner]).max()
        assert de <= 1e-9 * e.max() + ULP * base[3].max()
        d = got[0] - base[0]
        assert not d[:, :, D:, :].any() and not d[:, :, :, D:].any() and not (got[2] - base[2])[:, :, D:].any()
        h.close()
    pl.set_self_pairs(None)
    assert pl.self_pairs_count() == 0
    for x, y in zip(pl.linearize(traj), base):
        assert _bits(x, y)
    pl.close()


# --------------------------------------------------------------------------------------------------- 2. dist == 0
def test_coincident_centres_give_the_full_error_and_a_zero_row(engine, oracle):
    p, traj = mr.plan_case("wam")
    p.model, (a, b) = spr.duplicated_sphere_model()
    N, D = p.setting.total_step, p.setting.dof
    r, s, ro, so = _handles(engine, oracle, p)
    own, _ = engine.sphere_centers(r, traj[:, :, :D].reshape(-1, D))
    assert _bits(own[:, a], own[:, b])                           # equal bit for bit on the device
    eps, sigma = 0.05, 0.01
    q, pl = _plan(engine, r, s, p, 4, (1, N - 1))
    pl.set_problem(*_args(p), p.init)
    base = pl.linearize(traj)
    h = engine.self_pairs(r, [[a, b, eps, sigma]])
    pl.set_self_pairs(h)
    got = pl.linearize(traj)
    assert all(np.isfinite(x).all() for x in got)
    for k in (0, 1, 2):
        assert _bits(got[k], base[k])                            # nothing to G or g
    te = 2 * p.model.spheres[a].radius + eps
    want = (N - 1) * 0.5 * te * te / (sigma * sigma)             # w total_eps^2 per state in the record, r^T r / 2 in the error
    print(f"dist == 0: the error grows by {got[3] - base[3]}, reference {want}")
    np.testing.assert_allclose(got[3] - base[3], want, rtol=1e-9, atol=ULP * base[3].max())
    np.testing.assert_allclose(got[3], spr.linearize(oracle, ro, so, p, traj, dict(table=h.data, states=(1, N - 1)))[3], rtol=1e-9)
    h.close()
    pl.close()


# ------------------------------------------------------------------------------------ 3. P <= 16 through both routes
@pytest.mark.parametrize("name", ["wam", "config5"])
def test_sixteen_rows_agree_through_both_routes(engine, oracle, name):
    p, traj = mr.plan_case(name)
    N = p.setting.total_step
    r, s, ro, so = _handles(engine, oracle, p)
    table = spr.near_table(oracle, p.model, ro, traj, spr.case_ids(name, p.model))[:16]
    states = (1, N - 1)
    rows = copy.deepcopy(p)
    rows.setting.self_collision = table
    rows.setting.self_collision_states = states
    want = oracle.linearize(ro, so, rows.setting, *_args(p), traj)
    pl_rows = engine.plan(r, s, rows.setting, p.B)
    pl_rows.set_problem(*_args(p), p.init)
    _compare(pl_rows.linearize(traj), pl_rows.graph_error(traj), want, f"{name}: rows in the settings")
    pl_rows.close()
    q, pl = _plan(engine, r, s, p, 16, states)
    pl.set_problem(*_args(p), p.init)
    h = engine.self_pairs(r, table)
    pl.set_self_pairs(h)
    _compare(pl.linearize(traj), pl.graph_error(traj), want, f"{name}: the same rows as a table")
    h.close()
    pl.close()


@pytest.fixture(scope="module")
def motivation(engine, oracle):
    p = ref.motivation_inputs()[0][0]
    r, s, ro, so = _handles(engine, oracle, p)
    return dict(p=p, J=ref.motivation_inputs()[0][1], r=r, s=s, ro=ro, so=so, table=sr.wam_table(oracle, p.model, ro))


def _closest_sixteen(oracle, m):
    """the 16 pairs of the 78 that come closest on the initial values, at (0.05, 0.02)"""
    p = m["p"]
    c, _ = oracle.sphere_centers(m["ro"], np.ascontiguousarray(p.init[:, :, :7]).reshape(-1, 7))
    dist, te = sr.pair_clearance(p.model, c, m["table"][:, :2])
    keep = np.sort(np.argsort((dist - te).min(axis=0), kind="stable")[:16])
    t = m["table"][keep].copy()
    t[:, 2], t[:, 3] = 0.05, 0.02
    return t


@pytest.mark.parametrize("opt", ["GN", "LM", "DOGLEG"])
def test_sixteen_rows_solve_to_tolerance_as_the_oracle_does(engine, oracle, motivation, opt):
    """motivation input 0 (B = 16, N = 12): the table plan against oracle.batch_optimize with the same rows in its
    settings, under the parity contract"""
    m = motivation
    p = copy.deepcopy(m["p"])
    {"GN": lambda: None, "LM": p.setting.setLM, "DOGLEG": p.setting.setDogleg}[opt]()
    table = _closest_sixteen(oracle, m)
    rows = copy.deepcopy(p)
    rows.setting.self_collision = table
    want = oracle.batch_optimize(m["ro"], m["so"], rows.setting, *_args(p), p.init)
    q, pl = _plan(engine, m["r"], m["s"], p, 16)
    h = engine.self_pairs(m["r"], table)
    pl.set_self_pairs(h)
    h.close()
    pl.set_problem(*_args(p), p.init)
    pl.optimize()
    res = pl.result()
    pl.close()
    d = pb.per_traj_diff(res, want)
    print(f"{opt}: iters {res['iters']} / {want['iters']}, max |traj - oracle| per row {d}")
    assert list(res["iters"]) == list(want["iters"]) and list(res["status"]) == list(want["status"])
    over = np.nonzero(d > pb.CONTRACT)[0]
    if over.size:
        d_self = pb.oracle_self_sensitivity(oracle, (m["ro"], m["so"]), rows, want, over)
        print(f"{opt}: rows {over} above 1e-6: {d[over]}, the oracle's own 2-ulp sensitivity {d_self}")
        assert (d[over] <= pb.K_SELF * d_self).all()
    np.testing.assert_allclose(res["final_error"], oracle.graph_error(m["ro"], m["so"], rows.setting, *_args(p), res["traj"]),
                               rtol=1e-8)


# ---------------------------------------------------------------------------------- 4. solves with more than 16 pairs
@pytest.fixture(scope="module")
def scen(engine, oracle):
    p = spr.scenario()
    r, s, ro, so = _handles(engine, oracle, p)
    table = spr.wam_table(oracle, p.model, ro)
    assert len(table) == 78
    return dict(p=p, r=r, s=s, ro=ro, so=so, sp=dict(table=table, states=(0, p.setting.total_step)))


def _scenario_plan(engine, sc, p, B=None):
    q, pl = _plan(engine, sc["r"], sc["s"], p, 78, B=B)
    h = engine.self_pairs(sc["r"], sc["sp"]["table"])
    pl.set_self_pairs(h)
    h.close()
    return q, pl


def test_fixed_iteration_solve_equals_the_reference_loop(engine, oracle, scen):
    sc = scen
    p = copy.deepcopy(sc["p"])
    p.setting.fixed_iterations = spr.ITERS
    q, pl = _scenario_plan(engine, sc, p)
    pl.set_problem(*_args(q), q.init)
    pl.optimize()
    res = pl.result()
    want = spr.gauss_newton(oracle, sc["ro"], sc["so"], p, sc["sp"], spr.ITERS)
    plain = spr.gauss_newton(oracle, sc["ro"], sc["so"], p, None, spr.ITERS)
    d = np.abs(res["traj"] - want).max()
    print(f"GN x{spr.ITERS}: max |traj - reference| {d:.2e}; the factor moves the reference by {np.abs(want - plain).max():.2e}")
    assert list(res["iters"]) == [spr.ITERS] * p.B
    assert d <= 1e-6 and np.abs(want - plain).max() > 1e-2
    np.testing.assert_allclose(res["final_error"], spr.graph_error(oracle, sc["ro"], sc["so"], p, res["traj"], sc["sp"]), rtol=1e-8)
    pl.set_self_pairs(None)                                      # cleared: the same plan solves the plain problem
    pl.set_problem(*_args(q), q.init)
    pl.optimize()
    assert np.abs(pl.result()["traj"] - plain).max() <= 1e-6
    pl.close()


def test_queue_run_with_slot_refill_equals_the_reference_loop(engine, oracle, scen):
    """M = 5 problems through B = 3 slots"""
    sc = scen
    p5 = problems.wam_restarts(B=5, total_step=10, obs_check_inter=2, sdf="40")
    p5.setting.fixed_iterations = spr.ITERS
    q, pl = _scenario_plan(engine, sc, p5, B=3)
    res = pl.optimize_queue(*_args(q), q.init)
    want = spr.gauss_newton(oracle, sc["ro"], sc["so"], p5, sc["sp"], spr.ITERS)
    d = np.abs(res["traj"] - want).reshape(5, -1).max(axis=1)
    print(f"queue 5 through 3: max |traj - reference| per problem {d}")
    assert list(res["iters"]) == [spr.ITERS] * 5
    assert d.max() <= 1e-6
    pl.close()


@pytest.mark.parametrize("opt", ["LM", "DOGLEG"])
def test_lm_and_dogleg_report_the_error_with_the_factor(engine, oracle, scen, opt):
    sc = scen
    p = copy.deepcopy(sc["p"])
    {"LM": p.setting.setLM, "DOGLEG": p.setting.setDogleg}[opt]()
    q, pl = _scenario_plan(engine, sc, p)
    pl.set_problem(*_args(q), q.init)
    pl.optimize()
    res = pl.result()
    e_ref = spr.graph_error(oracle, sc["ro"], sc["so"], p, res["traj"], sc["sp"])
    e_plain = oracle.graph_error(sc["ro"], sc["so"], p.setting, *_args(p), res["traj"])
    print(f"{opt}: iters {res['iters']}, final_error {res['final_error']}, rel to the reference "
          f"{np.abs(res['final_error'] / e_ref - 1).max():.2e}; the factor's share {e_ref - e_plain}")
    np.testing.assert_allclose(res["final_error"], e_ref, rtol=1e-8)
    assert (res["iters"] >= 1).all()
    for b in range(p.B):
        tr = res["error_trace"][b]
        tr = tr[~np.isnan(tr)]
        assert tr.size >= 1 and (np.diff(tr) <= 0).all() and res["final_error"][b] <= tr[0], (b, tr)
    pl.close()


# ------------------------------------------------------------------------------------- 5. what the feature is for
def test_no_row_that_passes_the_obstacle_rule_touches_itself(engine, oracle, motivation):
    """motivation input 0, Gauss-Newton to tolerance: with the 78 pairs at (0.05, 0.005) on all support states no row
    that passes the obstacle rule touches itself (J = 4, table with epsilon 0); the plain plan has 9 of its 15."""
    m = motivation
    p, J = m["p"], m["J"]
    dt = ref.delta_t(p.setting)
    field = ref.oracle_sdf(oracle, p.sdf_origin, p.sdf_cell, p.sdf_data)
    check = engine.self_pairs(m["r"], m["table"])                # epsilon 0
    factor = m["table"].copy()
    factor[:, 2], factor[:, 3] = spr.EPSILON, spr.SIGMA
    counts = {}
    for label, table in (("plain", None), ("table", factor)):
        q, pl = _plan(engine, m["r"], m["s"], p, 78)
        if table is not None:
            h = engine.self_pairs(m["r"], table)
            pl.set_self_pairs(h)
            h.close()
        pl.set_problem(*_args(p), p.init)
        pl.optimize()
        res = pl.result()
        sp = None if table is None else dict(table=table, states=(0, p.setting.total_step))
        np.testing.assert_allclose(res["final_error"], spr.graph_error(oracle, m["ro"], m["so"], p, res["traj"], sp), rtol=1e-8)
        ob = ref.oracle_score(oracle, p.model, m["ro"], field, dt, J, res["traj"])
        se = sr.oracle_self_score(oracle, p.model, m["ro"], m["table"], dt, J, res["traj"])
        dev = pl.self_score(check, J)
        passing = scoring.eligible(res["final_error"], res["status"], ob["min_clearance"], ob["out_of_range"], 0.0, False)
        hit, hit_dev = passing & (se["min_self_clearance"] < 0.0), passing & (dev["min_self_clearance"] < 0.0)
        sel = pl.select_checked(J, check)
        counts[label] = (int(passing.sum()), int(hit.sum()), int(hit_dev.sum()), sel["n_eligible"])
        print(f"{label}: iters {res['iters']}; {passing.sum()} rows pass the obstacle rule, {hit.sum()} of them touch "
              f"themselves ({hit_dev.sum()} by the device's check); smallest self clearance of a passing row "
              f"{se['min_self_clearance'][passing].min():+.4f}; select_checked takes row {sel['best']} of {sel['n_eligible']}")
        pl.close()
    check.close()
    assert counts["plain"][:3] == (15, 9, 9)
    n_pass, n_hit, n_hit_dev, n_sel = counts["table"]
    assert n_pass > 0 and (n_hit, n_hit_dev) == (0, 0) and n_sel == n_pass


# --------------------------------------------------------------------------------- 6. errors that need a live plan
def test_errors_that_need_a_live_plan(engine, oracle, scen):
    sc = scen
    p, table = sc["p"], sc["sp"]["table"]
    r = sc["r"]
    q, pl = _plan(engine, r, sc["s"], p, 40)
    pl.set_problem(*_args(p), p.init)
    held = engine.self_pairs(r, table[:40])
    pl.set_self_pairs(held)
    before = pl.linearize(p.init)
    zero_sigma, nan_eps, inf_sigma = table[:3].copy(), table[:3].copy(), table[:3].copy()
    zero_sigma[1, 3], nan_eps[2, 2], inf_sigma[0, 3] = 0.0, np.nan, np.inf
    arm3 = problems.arm3_planner().model
    r3 = engine.robot(arm3)
    other = engine.self_pairs(r3, spr.near_table(oracle, arm3, oracle.robot(arm3), np.zeros((1, 2, 6)), sr.candidate_pairs(arm3, 2)[:4]))
    for label, h in (("above the capacity", engine.self_pairs(r, table[:41])), ("another robot", other),
                     ("sigma 0", engine.self_pairs(r, zero_sigma)), ("NaN epsilon", engine.self_pairs(r, nan_eps)),
                     ("sigma inf", engine.self_pairs(r, inf_sigma))):
        with pytest.raises(E.Gpmp2miError) as ei:
            pl.set_self_pairs(h)
        assert ei.value.code == 1, label
        assert pl.self_pairs_count() == 40, label
        h.close()
    for x, y in zip(before, pl.linearize(p.init)):               # the plan holds what it held
        assert _bits(x, y)
    pl.optimize()                                                # and still solves
    assert (pl.result()["iters"] >= 1).all()
    # the table handle may go as soon as the call returns
    alive = pl.result()
    held.close()
    pl.set_problem(*_args(p), p.init)
    pl.optimize()
    gone = pl.result()
    for k in ("traj", "final_error", "iters", "status"):
        assert _bits(alive[k], gone[k]) if alive[k].dtype == np.float64 else np.array_equal(alive[k], gone[k]), k
    pl.close()
    # a plan created without capacity takes no table, not even an empty one
    pl0 = engine.plan(r, sc["s"], p.setting, p.B)
    h = engine.self_pairs(r, table[:2])
    for arg in (h, None):
        with pytest.raises(E.Gpmp2miError) as ei:
            pl0.set_self_pairs(arg)
        assert ei.value.code == 1 and "without room" in str(ei.value)
    assert pl0.self_pairs_count() == 0
    h.close()
    pl0.close()
    # creation: the fields are validated before anything is allocated
    N = p.setting.total_step
    for cap, states in ((-1, None), (_capi.MAX_PLAN_SELF_PAIRS + 1, None), (2, (3, 2)), (2, (0, N + 1)), (2, (-1, 2))):
        st, o, keep = _capi.make_settings(p.setting)
        o.max_self_pairs = cap
        o.self_pairs_first, o.self_pairs_last = states or (0, N)
        out = C.c_void_p()
        assert engine.lib.gpmp2mi_plan_create(r.ptr, sc["s"].ptr, C.byref(st), C.byref(o), p.B, C.byref(out)) == 1, (cap, states)
        assert out.value is None and len(engine.lib.gpmp2mi_last_error()) > 0


# ------------------------------------------------------------------------ 7. plans without capacity are left alone
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
    o.max_self_pairs = 0
    o.self_pairs_first, o.self_pairs_last = 7, -3                # not read without capacity
    return o


def _zeros(o):
    o.max_self_pairs = o.self_pairs_first = o.self_pairs_last = 0
    return o


@pytest.mark.parametrize("kind", ["default", "extras"])
def test_plans_without_capacity_are_left_alone(engine, kind):
    """a plan created with the default graph_opts, and one that carries workspace / self-collision factors but no
    capacity: bit-identical to their twins created from a struct whose new fields are explicitly zero"""
    if kind == "default":
        p = problems.wam_restarts(B=3, total_step=10, obs_check_inter=2, sdf="40")
        edits = (lambda o: None, _zeros, _junk_without_capacity)
    else:
        p = problems.wam_restarts(B=3, total_step=10, obs_check_inter=2, sdf="40", opt="LM")
        p.setting.self_collision = np.array([[0, 9, 0.6, 0.05], [1, 15, 0.5, 0.1], [5, 12, 0.4, 0.05]])
        p.setting.self_collision_states = (1, 9)
        des = np.eye(4)
        des[:3, 3] = [0.4, 0.3, 0.5]
        p.setting.add_workspace_prior(0, 6, des, 0.05, 5)
        edits = (lambda o: o, _zeros, _junk_without_capacity)
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    results = []
    for edit in edits:
        pl = _plan_with_opts(engine, r, s, p.setting, p.B, edit)
        pl.set_problem(*_args(p), p.init)
        pl.optimize()
        results.append(pl.result())
        pl.close()
    assert (results[0]["iters"] >= 1).all()
    for other in results[1:]:
        for k in ("traj", "final_error", "iters", "status"):
            assert np.array_equal(results[0][k], other[k]), (kind, k)
