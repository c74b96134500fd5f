"""Moving obstacles on the device (include/gpmp2mi.h "moving obstacles") against the numpy reference on the CPU oracle
(tests/moving_reference.py): the factor, the plan's normal equations and graph error with the factor, whole solves
(Gauss-Newton, queue runs, LM, Dogleg), the check of the executed trajectory with its selection, the argument and state
errors that need a live plan, and that plans without capacity are left alone.

Tolerances are the project's own: normal equations atol 1e-9 max|ref|, errors rtol 1e-9, costs rtol 1e-8 / atol 1e-12,
clearances atol 1e-9, final error rtol 1e-8, solved trajectories 1e-6."""
import copy
import ctypes as C

import numpy as np
import pytest

import moving_reference as mr
import score_reference as ref
from gpmp2_amd import _capi, problems, scoring
from gpmp2_amd import engine as E

pytestmark = pytest.mark.gpu
FIVE = scoring.MOVING_NAMES


def _args(p):
    return p.start_conf, p.start_vel, p.end_conf, p.end_vel


def _same_bits(a, b, rows=None, what="", names=FIVE):
    """the outputs agree bit for bit (rows: (rows of a, rows of b))"""
    for k in names:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows[0]], b[k][rows[1]])
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.dtype == np.float64:
            x, y = x.view(np.int64), y.view(np.int64)
        assert np.array_equal(x, y), (what, k, a[k], b[k])


def _handles(engine, oracle, p):
    return (engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data),
            oracle.robot(p.model), oracle.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data))


# ------------------------------------------------------------------------------------------------ 6. the factor
@pytest.mark.parametrize("K", [1, 4, 5])
@pytest.mark.parametrize("name", ["arm3", "wam", "config5"])
def test_factor_matches_the_reference(engine, oracle, name, K):
    """S K sits below, on and above a 64-pair chunk for the WAM (S = 16).  The centres are the reference's sphere centres
    plus an offset of known length, so both hinge branches occur; one pair has dist == 0 on the device."""
    p, traj = mr.plan_case(name)
    model, D = p.model, p.setting.dof
    r, ro = engine.robot(model), oracle.robot(model)
    radius, centers = mr.spheres_near(oracle, model, ro, traj, K, 20 + K, mr.EPSILON)
    conf = np.ascontiguousarray(traj[0, :, :D])
    cen = np.ascontiguousarray(centers.transpose(1, 0, 2))          # [M][K][3]
    # dist == 0: moving sphere 0 of evaluation 0 sits on the DEVICE's centre of body sphere 2, bit for bit
    own, _ = engine.sphere_centers(r, conf[:1])
    cen[0, 0] = own[0, 2]
    err, H = engine.moving_sphere_factor(r, radius, mr.EPSILON, conf, cen)
    e_ref, H_ref, dist = mr.hinge_rows(oracle, model, ro, conf, radius, cen, mr.EPSILON)
    te = mr.total_eps(model, radius, mr.EPSILON)
    assert err[0, 2, 0] == te[2, 0] and (H[0, 2, 0] == 0.0).all()     # err = total_eps, a zero row
    assert np.isfinite(err).all() and np.isfinite(H).all()             # no NaN is made
    assert (e_ref > 0).any() and (e_ref == 0).any()                    # both branches of the hinge
    assert ((e_ref > 0) == (err > 0)).all()
    mask = np.ones(err.shape, dtype=bool)
    mask[0, 2, 0] = False                                              # the reference's direction there is rounding noise
    assert dist[0, 2, 0] < 1e-12
    de = np.abs(err - e_ref)[mask].max()
    dH = np.abs(H - H_ref)[mask].max()
    print(f"{name} K={K}: {int((e_ref > 0).sum())} of {e_ref.size} rows active, max |d err| {de:.2e}, max |d H| {dH:.2e}")
    np.testing.assert_allclose(err[mask], e_ref[mask], rtol=1e-9, atol=0)
    np.testing.assert_allclose(err[0, 2, 0], e_ref[0, 2, 0], rtol=1e-9)
    assert dH <= 1e-9 * np.abs(H_ref).max()
    e_only, none = engine.moving_sphere_factor(r, radius, mr.EPSILON, conf, cen, jac=False)
    assert none is None and np.array_equal(e_only.view(np.int64), err.view(np.int64))


# ------------------------------------------------------------------------------------ 7. linearize and graph error
def _compare_linearize(pl, oracle, ro, so, p, traj, mv, label):
    a = pl.linearize(traj)
    b = mr.linearize(oracle, ro, so, p, traj, mv)
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


@pytest.mark.parametrize("name", mr.PLAN_CASES)
def test_plan_linearize_and_graph_error_carry_the_factor(engine, oracle, name):
    """B = 3, states (1, N - 1): narrow (arm3, WAM, config5: Pose2 chart), wide (mobile WAM, dof 10) and dense (PR2)
    blocks.  K = 0 is oracle.linearize alone; two sets in a row are both reflected without recreating the plan."""
    p, traj = mr.plan_case(name)
    N = p.setting.total_step
    p.setting.set_moving_spheres(8, mr.EPSILON, mr.SIGMA, states=(1, N - 1))
    r, s, ro, so = _handles(engine, oracle, p)
    pl = engine.plan(r, s, p.setting, p.B)
    pl.set_problem(*_args(p), p.init)
    D = p.setting.dof
    base, _ = _compare_linearize(pl, oracle, ro, so, p, traj, None, f"{name} K=0")
    for K, seed in ((5, 31), (3, 32)):
        radius, centers = mr.spheres_near(oracle, p.model, ro, traj, K, seed, mr.EPSILON)
        mv = dict(radius=radius, centers=centers, epsilon=mr.EPSILON, sigma=mr.SIGMA, states=(1, N - 1))
        pl.set_moving_spheres(radius, centers)
        G, gg, e = mr.plan_terms(oracle, p.model, ro, traj, radius, centers, mr.EPSILON, mr.SIGMA, (1, N - 1))
        assert (e > 0).all() and np.abs(G).max() > 0          # the factor is on in every row
        got, want = _compare_linearize(pl, oracle, ro, so, p, traj, mv, f"{name} K={K}")
        for x, y in zip(got, pl.linearize(traj)):
            assert np.array_equal(x.view(np.int64), y.view(np.int64))         # the same bits on a second run
        # states outside the range are untouched: their blocks are those of the plan without spheres
        for i in (0, N):
            assert np.array_equal(got[0][:, i].view(np.int64), base[0][:, i].view(np.int64)), i
            assert np.array_equal(got[2][:, i].view(np.int64), base[2][:, i].view(np.int64)), i
        # The factor's own share, free of the 1e8 priors of states 0 and N that set the scale of the bound above: what
        # the spheres add to the blocks of states 1 .. N - 1 against the reference terms.  Bound: the project's 1e-9 of
        # the terms, plus the cancellation of the subtraction (a few ulp of the interior blocks).
        inner = slice(1, N)
        ulp = 8 * np.finfo(np.float64).eps
        dG = np.abs((got[0] - base[0])[:, inner, :D, :D] - G[:, inner]).max()
        dg = np.abs((got[2] - base[2])[:, inner, :D] - gg[:, inner]).max()
        de = np.abs((got[3] - base[3]) - e).max()
        print(f"{name} K={K}: the factor's share: |d G| {dG:.2e} of {np.abs(G).max():.2e}, |d g| {dg:.2e} of "
              f"{np.abs(gg).max():.2e}, |d e| {de:.2e} of {e.max():.2e}")
        assert dG <= 1e-9 * np.abs(G).max() + ulp * np.abs(base[0][:, inner]).max()
        assert dg <= 1e-9 * np.abs(gg).max() + ulp * np.abs(base[2][:, inner]).max()
        assert de <= 1e-9 * e.max() + ulp * base[3].max()
        assert np.array_equal((got[0] - base[0])[:, :, D:, :], np.zeros_like(got[0][:, :, D:, :]))   # velocities: nothing
    pl.close()


# -------------------------------------------------------------------------------------------------- 8. the solves
@pytest.fixture(scope="module")
def scen(engine, oracle):
    p, mv = mr.scenario()
    r, s, ro, so = _handles(engine, oracle, p)
    mv = dict(mv, centers=mr.scenario_centers(oracle, ro, p, mv))
    return dict(p=p, mv=mv, r=r, s=s, ro=ro, so=so)


def _scenario_plan(engine, sc, p, B=None):
    q = copy.deepcopy(p)
    q.setting.set_moving_spheres(2, sc["mv"]["epsilon"], sc["mv"]["sigma"])
    pl = engine.plan(sc["r"], sc["s"], q.setting, B or q.B)
    pl.set_moving_spheres(sc["mv"]["radius"], sc["mv"]["centers"])
    return q, pl


def test_fixed_iteration_solve_equals_the_reference_loop(engine, oracle, scen):
    sc = scen
    p = copy.deepcopy(sc["p"])
    p.setting.fixed_iterations = mr.ITERS
    q, pl = _scenario_plan(engine, sc, p)
    pl.set_problem(*_args(q), q.init)
    pl.optimize()
    res = pl.result()
    want = mr.gauss_newton(oracle, sc["ro"], sc["so"], p, sc["mv"], mr.ITERS)
    plain = mr.gauss_newton(oracle, sc["ro"], sc["so"], p, None, mr.ITERS)
    d = np.abs(res["traj"] - want).max()
    print(f"GN x{mr.ITERS}: max |traj - reference| {d:.2e}; the factor moves the reference by {np.abs(want - plain).max():.2e}")
    assert list(res["iters"]) == [mr.ITERS] * p.B
    assert d <= 1e-6 and np.abs(want - plain).max() > 1e-2
    e_ref = mr.graph_error(oracle, sc["ro"], sc["so"], p, res["traj"], sc["mv"])
    np.testing.assert_allclose(res["final_error"], e_ref, rtol=1e-8)
    # cleared set: the same plan solves the problem without the factor
    pl.set_moving_spheres(None, None)
    pl.set_problem(*_args(q), q.init)
    pl.optimize()
    assert np.abs(pl.result()["traj"] - plain).max() <= 1e-6
    pl.close()


def test_queue_run_with_slot_refill_equals_the_reference_loop(engine, oracle, scen):
    """M = 5 problems through B = 3 slots"""
    sc = scen
    p5 = problems.wam_restarts(B=5, total_step=10, obs_check_inter=2, sdf="40")
    p5.setting.fixed_iterations = mr.ITERS
    q, pl = _scenario_plan(engine, sc, p5, B=3)
    res = pl.optimize_queue(*_args(q), q.init)
    want = mr.gauss_newton(oracle, sc["ro"], sc["so"], p5, sc["mv"], mr.ITERS)
    d = np.abs(res["traj"] - want).reshape(5, -1).max(axis=1)
    print(f"queue 5 through 3: max |traj - reference| per problem {d}")
    assert list(res["iters"]) == [mr.ITERS] * 5
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
    e_ref = mr.graph_error(oracle, sc["ro"], sc["so"], p, res["traj"], sc["mv"])
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


# ---------------------------------------------------------------------------------------------------- 9. the check
def _check_against_reference(dev, exp, label):
    B = len(exp["invalid"])
    finite = np.isfinite(exp["min_moving_clearance"])
    dclr = np.abs(dev["min_moving_clearance"][finite] - exp["min_moving_clearance"][finite]).max() if finite.any() else 0.0
    print(f"{label}: max |d support| {np.abs(dev['moving_support_cost'] - exp['moving_support_cost']).max():.2e}, "
          f"max |d dense| {np.abs(dev['moving_dense_cost'] - exp['moving_dense_cost']).max():.2e}, "
          f"max |d clearance| {dclr:.2e}, gaps {exp['gap']}")
    np.testing.assert_allclose(dev["moving_support_cost"], exp["moving_support_cost"], rtol=1e-8, atol=1e-12, err_msg=label)
    np.testing.assert_allclose(dev["moving_dense_cost"], exp["moving_dense_cost"], rtol=1e-8, atol=1e-12, err_msg=label)
    np.testing.assert_allclose(dev["min_moving_clearance"], exp["min_moving_clearance"], rtol=0, atol=1e-9, err_msg=label)
    assert np.array_equal(dev["invalid"], exp["invalid"]), (label, dev["invalid"], exp["invalid"])
    # worst: the reference's argmin wherever its runner-up is more than 1e-6 above the minimum; a closer row whose
    # triple differs is excused, at most 10 % of the rows (tests/test_moving_cpu.py: the inputs keep to that)
    with np.errstate(invalid="ignore"):
        decided = ~(exp["gap"] <= 1e-6)
    differs = (dev["worst"] != exp["worst"]).any(axis=1)
    assert not (differs & decided).any(), (label, dev["worst"][differs], exp["worst"][differs], exp["gap"][differs])
    assert differs.sum() <= 0.1 * B, (label, "rows excused", int(differs.sum()), B)


@pytest.fixture(scope="module")
def check_robots(engine, oracle):
    made = {}

    def get(name):
        if name not in made:
            model = mr.check_models()[name]()
            made[name] = (model, engine.robot(model), oracle.robot(model))
        return made[name]
    return get


@pytest.mark.parametrize("case", mr.CHECK_CASES, ids=[mr.check_id(c) for c in mr.CHECK_CASES])
def test_check_matches_the_reference(engine, oracle, check_robots, case):
    name, (N, J), K = case
    model, r, ro = check_robots(name)
    traj = mr.check_traj(name, N)
    assert traj.shape[0] == 3
    radius, centers = mr.spheres_near(oracle, model, ro, traj, K, 17 + K, mr.EPSILON)
    exp = mr.oracle_moving_score(oracle, model, ro, radius, centers, mr.EPSILON, mr.CHECK_DT, J, traj)
    dev = engine.moving_score_traj(r, radius, centers, mr.EPSILON, mr.CHECK_DT, J, traj)
    _check_against_reference(dev, exp, mr.check_id(case))
    if J == 0:   # the support states are all there is: the two sums are the same additions
        assert np.array_equal(dev["moving_dense_cost"].view(np.int64), dev["moving_support_cost"].view(np.int64))
    if K == 0:
        assert (dev["moving_dense_cost"] == 0.0).all() and np.isposinf(dev["min_moving_clearance"]).all()
        assert (dev["worst"] == -1).all() and (dev["invalid"] == 0).all()
    else:
        assert (dev["moving_dense_cost"] > 0).any() and (dev["min_moving_clearance"] < 0).any()
    # a row alone, and in another batch at another position: the same bits
    alone = engine.moving_score_traj(r, radius, centers, mr.EPSILON, mr.CHECK_DT, J, traj[1])
    _same_bits(alone, dev, rows=(0, 1), what="alone vs row 1 of 3")
    other = np.concatenate([traj[2:], traj[:1], traj[1:2], traj[:2]])
    _same_bits(engine.moving_score_traj(r, radius, centers, mr.EPSILON, mr.CHECK_DT, J, other), dev, rows=(2, 1),
               what="row 2 of 5 vs row 1 of 3")
    if K:
        # a NaN row is invalid and leaves its neighbours' bits alone
        bad = traj.copy()
        bad[1] = np.nan
        sc = engine.moving_score_traj(r, radius, centers, mr.EPSILON, mr.CHECK_DT, J, bad)
        Md = scoring.checked_states(N, J)
        assert sc["invalid"][1] == Md * model.nr_body_spheres() * K
        assert sc["moving_dense_cost"][1] == 0.0 and sc["moving_support_cost"][1] == 0.0
        assert np.isposinf(sc["min_moving_clearance"][1]) and tuple(sc["worst"][1]) == (-1, -1, -1)
        _same_bits(sc, dev, rows=([0, 2], [0, 2]), what="ordinary rows beside a NaN row")


@pytest.fixture(scope="module")
def solved(engine, oracle, scen):
    """the scenario solved on the device WITHOUT the spheres (an empty set), then given them: rows that touch them"""
    sc = scen
    p = copy.deepcopy(sc["p"])
    p.setting.fixed_iterations = mr.ITERS
    q = copy.deepcopy(p)
    q.setting.set_moving_spheres(4, sc["mv"]["epsilon"], sc["mv"]["sigma"])
    pl = engine.plan(sc["r"], sc["s"], q.setting, q.B)
    pl.set_problem(*_args(q), q.init)
    pl.optimize()
    res = pl.result()
    pl.set_moving_spheres(sc["mv"]["radius"], sc["mv"]["centers"])
    return dict(sc, pl=pl, res=res, q=q, dt=ref.delta_t(q.setting))


def test_the_plan_form_scores_the_same_bits_as_the_trajectory_form(engine, oracle, solved):
    w = solved
    pl, mv, traj = w["pl"], w["mv"], w["res"]["traj"]
    for J in (0, 2, 3):
        through_plan = pl.moving_score(J)
        exp = mr.oracle_moving_score(oracle, w["p"].model, w["ro"], mv["radius"], mv["centers"], mv["epsilon"], w["dt"], J, traj)
        _check_against_reference(through_plan, exp, f"scenario through the plan, J={J}")
        batch = engine.moving_score_traj(w["r"], mv["radius"], mv["centers"], mv["epsilon"], w["dt"], J, traj)
        _same_bits(through_plan, batch, what="Plan.moving_score vs Engine.moving_score_traj on the fetched result")
        _same_bits(through_plan, pl.moving_score(J), what="Plan.moving_score twice in a row")
    assert through_plan["min_moving_clearance"].min() < -mv["epsilon"]       # a row is in contact with a sphere
    part = pl.moving_score(3, out={"min_moving_clearance": np.zeros(3)})
    assert np.array_equal(part["min_moving_clearance"].view(np.int64), through_plan["min_moving_clearance"].view(np.int64))


def test_select_moving_is_the_extended_rule_on_the_reference_scores(engine, oracle, solved):
    w = solved
    pl, mv, res, J = w["pl"], w["mv"], w["res"], 2
    p = w["p"]
    field = ref.oracle_sdf(oracle, p.sdf_origin, p.sdf_cell, p.sdf_data)
    ob = ref.oracle_score(oracle, p.model, w["ro"], field, w["dt"], J, res["traj"])
    mo = mr.oracle_moving_score(oracle, p.model, w["ro"], mv["radius"], mv["centers"], mv["epsilon"], w["dt"], J, res["traj"])
    plain = pl.select(J, -np.inf, False)
    b0 = plain["best"]
    assert b0 >= 0 and plain["n_eligible"] == 3
    # a threshold that only the best row by error fails, or that it fails first: just above its moving clearance
    clr = mo["min_moving_clearance"]
    thr = clr[b0] + 1e-3
    assert (np.abs(clr - thr) > 1e-6).all()
    want = scoring.moving_rule(res["final_error"], res["status"], ob["min_clearance"], ob["out_of_range"], -np.inf, False,
                               min_moving_clearance=clr, moving_invalid=mo["invalid"], required_moving_clearance=thr)
    got = pl.select_moving(J, thr, required_clearance=-np.inf)
    print(f"select {b0} of {plain['n_eligible']}; moving clearances {clr}; select_moving(>= {thr:.4f}) {got['best']} of "
          f"{got['n_eligible']}, reference {want}")
    assert (got["best"], got["n_eligible"]) == want and want[0] != b0
    if want[0] >= 0:
        assert np.array_equal(got["traj_best"].view(np.int64), res["traj"][want[0]].view(np.int64))
    # several thresholds, with and without a pair table, against the rule applied to the reference scores
    pairs = engine.generate_self_pairs(w["r"], 2, np.zeros((1, 7)))
    import self_reference as sr
    se = sr.oracle_self_score(oracle, p.model, w["ro"], pairs.data, w["dt"], J, res["traj"])
    for req, rir, req_self, req_mv, with_pairs in ((0.0, True, 0.0, -np.inf, False), (-np.inf, False, -np.inf, -0.25, True),
                                                   (-np.inf, False, 0.0, float(np.sort(clr)[1]) - 1e-3, True),
                                                   (0.0, False, 0.0, 10.0, False)):
        a = pl.select_moving(J, req_mv, required_clearance=req, require_in_range=rir,
                             pairs=pairs if with_pairs else None, required_self_clearance=req_self)
        b = scoring.moving_rule(res["final_error"], res["status"], ob["min_clearance"], ob["out_of_range"], req, rir,
                                se["min_self_clearance"] if with_pairs else None, se["invalid"] if with_pairs else None,
                                req_self, clr, mo["invalid"], req_mv)
        assert (a["best"], a["n_eligible"]) == b, (req, rir, req_self, req_mv, with_pairs, a["best"], a["n_eligible"], b)
    none = pl.select_moving(J, 10.0, required_clearance=-np.inf)
    assert (none["best"], none["n_eligible"]) == (-1, 0) and none["traj_best"] is None and none["dense_best"] is None
    # K = 0 and -inf: the answer of the existing call
    pl.set_moving_spheres(None, None)
    for req, rir in ((-np.inf, False), (0.0, True)):
        a, b = pl.select_moving(J, -np.inf, required_clearance=req, require_in_range=rir), pl.select(J, req, rir)
        assert (a["best"], a["n_eligible"]) == (b["best"], b["n_eligible"])
        if b["best"] >= 0:
            assert np.array_equal(a["dense_best"].view(np.int64), b["dense_best"].view(np.int64))
    empty = pl.moving_score(J)
    assert np.isposinf(empty["min_moving_clearance"]).all() and (empty["worst"] == -1).all()
    pl.set_moving_spheres(mv["radius"], mv["centers"])
    pairs.close()


class _DevArray:
    """a device buffer from the library's own HIP runtime (gpmp2mi_debug_device_*): no second runtime in the process"""

    def __init__(self, engine, shape, dtype, fill_byte=0, data=None):
        self.eng, self.host = engine, np.zeros(shape, dtype=dtype)
        self.p = C.c_void_p()
        engine._ck(engine.lib.gpmp2mi_debug_device_alloc(C.c_size_t(self.host.nbytes), fill_byte, C.byref(self.p)))
        if data is not None:
            src = np.ascontiguousarray(data, dtype=dtype).reshape(shape)
            engine._ck(engine.lib.gpmp2mi_debug_device_write(self.p, src.ctypes.data_as(C.c_void_p), C.c_size_t(src.nbytes)))

    @property
    def ptr(self):
        return self.p.value

    def read(self):
        self.eng._ck(self.eng.lib.gpmp2mi_debug_device_read(self.host.ctypes.data_as(C.c_void_p), self.p,
                                                            C.c_size_t(self.host.nbytes)))
        return self.host.copy()

    def free(self):
        self.eng._ck(self.eng.lib.gpmp2mi_debug_device_free(self.p))


def test_the_dev_forms_take_and_write_device_buffers(engine, solved):
    w = solved
    pl, mv, J, B = w["pl"], w["mv"], 2, 3
    N, D = w["q"].setting.total_step, w["q"].setting.dof
    Md = scoring.checked_states(N, J)
    host = pl.moving_score(J)
    want = pl.select_moving(J, -0.25, required_clearance=-np.inf)
    rad = _DevArray(engine, (2,), np.float64, data=mv["radius"])
    cen = _DevArray(engine, (2, N + 1, 3), np.float64, data=mv["centers"])
    pl.set_moving_spheres(None, None)
    pl.set_moving_spheres_dev(2, rad.ptr, cen.ptr)
    FILL = 0x7B
    best, n = _DevArray(engine, (1,), np.int32, FILL), _DevArray(engine, (1,), np.int32, FILL)
    tb, db = _DevArray(engine, (N + 1, 2 * D), np.float64, FILL), _DevArray(engine, (Md, 2 * D), np.float64, FILL)
    clr, inv, worst = (_DevArray(engine, (B,), np.float64, FILL), _DevArray(engine, (B,), np.int32, FILL),
                       _DevArray(engine, (B, 3), np.int32, FILL))
    untouched = tb.read()
    pl.select_moving_dev(J, 10.0, required_clearance=-np.inf, best=best.ptr, n_eligible=n.ptr, traj_best=tb.ptr, dense_best=db.ptr)
    pl.moving_score_dev(J, min_moving_clearance=clr.ptr, invalid=inv.ptr, worst=worst.ptr)
    again = pl.moving_score(J)                          # waits for the null stream
    _same_bits(again, host, what="the set given through device buffers")
    assert (int(best.read()[0]), int(n.read()[0])) == (-1, 0)
    assert np.array_equal(tb.read().view(np.int64), untouched.view(np.int64))
    assert np.array_equal(clr.read().view(np.int64), host["min_moving_clearance"].view(np.int64))
    assert np.array_equal(inv.read(), host["invalid"]) and np.array_equal(worst.read(), host["worst"])
    pl.select_moving_dev(J, -0.25, required_clearance=-np.inf, best=best.ptr, n_eligible=n.ptr, traj_best=tb.ptr, dense_best=db.ptr)
    pl.moving_score(J)
    assert (int(best.read()[0]), int(n.read()[0])) == (want["best"], want["n_eligible"]) and want["best"] >= 0
    assert np.array_equal(tb.read().view(np.int64), want["traj_best"].view(np.int64))
    assert np.array_equal(db.read().view(np.int64), want["dense_best"].view(np.int64))
    for b in (rad, cen, best, n, tb, db, clr, inv, worst):
        b.free()


def test_errors_that_need_a_live_plan(engine, scen):
    sc = scen
    p, mv = sc["p"], sc["mv"]
    lib = engine.lib
    q, pl = _scenario_plan(engine, sc, p)       # capacity 2, the scenario's set resident
    N = p.setting.total_step
    for call in (lambda: pl.moving_score(1), lambda: pl.select_moving(1)):     # nothing to score yet
        with pytest.raises(E.Gpmp2miError) as ei:
            call()
        assert ei.value.code == 1 and "not been optimized" in str(ei.value)
    pl.set_problem(*_args(q), q.init)
    before = pl.linearize(q.init)
    # refused calls change nothing: over the capacity, a non-finite centre, a negative / non-finite radius
    three = np.concatenate([mv["centers"], mv["centers"][:1]])
    bad_c = mv["centers"].copy()
    bad_c[1, 3, 2] = np.inf
    for radius, centers in ((np.full(3, 0.05), three), (mv["radius"], bad_c), (np.array([0.05, -0.01]), mv["centers"]),
                            (np.array([np.nan, 0.05]), mv["centers"])):
        with pytest.raises(E.Gpmp2miError) as ei:
            pl.set_moving_spheres(radius, centers)
        assert ei.value.code == 1
    after = pl.linearize(q.init)
    for x, y in zip(before, after):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))
    assert lib.gpmp2mi_plan_set_moving_spheres(pl.h.ptr, 1, None, E.dptr(mv["centers"])) == 1
    assert lib.gpmp2mi_plan_set_moving_spheres(pl.h.ptr, -1, E.dptr(mv["radius"]), E.dptr(mv["centers"])) == 1
    pl.optimize()
    assert lib.gpmp2mi_plan_moving_score(pl.h.ptr, -1, None, None, None, None, None) == 1
    assert lib.gpmp2mi_plan_moving_score(pl.h.ptr, 1, None, None, None, None, None) == 0      # every output may be NULL
    pl.close()
    # a plan created without capacity: an empty set is all it takes, and it has no check
    pl0 = engine.plan(sc["r"], sc["s"], p.setting, p.B)
    pl0.set_problem(*_args(p), p.init)
    pl0.optimize()
    pl0.set_moving_spheres(None, None)
    with pytest.raises(E.Gpmp2miError) as ei:
        pl0.set_moving_spheres(mv["radius"][:1], mv["centers"][:1])
    assert ei.value.code == 1
    for call in (lambda: pl0.moving_score(1), lambda: pl0.select_moving(1)):
        with pytest.raises(E.Gpmp2miError) as ei:
            call()
        assert ei.value.code == 1 and "without room" in str(ei.value)
    pl0.close()
    # creation: the fields are validated before anything is allocated
    for cap, eps, sigma, states in ((65, 0.2, 0.01, None), (-1, 0.2, 0.01, None), (2, 0.2, 0.0, None), (2, np.inf, 0.01, None),
                                    (2, 0.2, 0.01, (3, 2)), (2, 0.2, 0.01, (0, N + 1)), (2, 0.2, 0.01, (-1, 2))):
        st, o, keep = _capi.make_settings(p.setting)
        o.max_moving_spheres, o.moving_epsilon, o.moving_sigma = cap, eps, sigma
        o.moving_first, o.moving_last = states or (0, N)
        out = C.c_void_p()
        assert lib.gpmp2mi_plan_create(sc["r"].ptr, sc["s"].ptr, C.byref(st), C.byref(o), p.B, C.byref(out)) == 1, (cap, eps, sigma, states)
        assert out.value is None


# ------------------------------------------------------------------------------- 10. the existing calls are left alone
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
    o.max_moving_spheres = 0
    o.moving_first, o.moving_last, o.moving_epsilon, o.moving_sigma = 7, 3, np.nan, -1.0     # not read without capacity
    return o


def _zeros(o):
    o.max_moving_spheres = o.moving_first = o.moving_last = 0
    o.moving_epsilon = o.moving_sigma = 0.0
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
