"""Re-timing under torque limits on the device (include/gpmp2mi.h "re-timing under torque limits") through every entry
point.

 1. gpmp2mi_retime_path_affine against gpmp2_amd/csrc/retime_affine_rule.h built by the host compiler
    (tests/retime_affine_shim.py): every output bit for bit on the inputs of tests/test_retime_dynamic_cpu.py, rows that
    are STATIC, EMPTY, BOUNDARY and INVALID in one batch, and every row against the same row alone.
 2. coef against a truth in np.longdouble, with the error form of tests/torque_reference.py:
    err = |x - truth| / max(1, |truth|), e_gpu <= K * max(e_cpu, FLOOR) and e_gpu <= CAP, where e_cpu is the float64
    link-frame reference's own error (K below; measured table: scripts/retime_dynamic_error.py ->
    profiles/retime_dynamic_error.txt).  Exact zeros: p == 0 wherever q' == 0.
 3. gpmp2mi_retime_dynamic_traj against the numpy rule (tests/retime_dynamic_reference.py) with coefficients from
    torque_reference.inverse_dynamics: sdot, stamps and duration within max(1e-12 relative, 10 x the numpy rule's own
    change under a 2-ulp perturbation of traj), the clause of tests/test_gpu_retime.py.  No more than one row in twenty
    may need the second clause; the test prints and asserts the count.
 4. the properties of the rule recomputed in numpy from the device's own coef, sdot and u; with every torque limit +inf
    the bits of gpmp2mi_retime_traj.
 5. the plan form, the `_dev` forms, the selection, the statuses, the refusals, and that the existing calls are left
    alone."""
import ctypes as C

import numpy as np
import pytest

import motion_reference as mr
import retime_affine_shim as shim
import retime_dynamic_reference as dr
import retime_reference as rr
import score_reference as ref
import torque_reference as tq
from gpmp2_amd import _capi, scoring
from gpmp2_amd import dynamics as tables
from gpmp2_amd import engine as E

pytestmark = pytest.mark.gpu
PATH_CASES = rr.path_cases()
MAX_RATE = 4.0
VEL = 3.0
PROFILE = ("sdot", "u", "stamps", "duration", "status", "achieved")
NAMES = scoring.RETIME_DYNAMIC_NAMES
# coef against the truth: the next power of two above the largest e_gpu / max(e_cpu, FLOOR) of
# profiles/retime_dynamic_error.txt (scripts/retime_dynamic_error.py), as torque_reference.K is set from
# profiles/torque_error.txt; FLOOR and CAP are the project's conditions
K, FLOOR, CAP = 32.0, tq.FLOOR, tq.CAP


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same_bits(a, b, names, rows=None, what=""):
    for k in names:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows[0]], b[k][rows[1]])
        assert np.array_equal(_bits(x), _bits(y)), (what, k, x, y)


def _dynamics(engine, r, table):
    return engine.dynamics(r, table["mass"], table["com"], table["inertia"], table["gravity"], table.get("torque"))


# ---------------------------------------------------------------------------------------------------------- the bare rule
@pytest.mark.parametrize("name", [n for n, _ in PATH_CASES])
def test_retime_path_affine_gives_the_bits_of_the_host_rule(engine, name):
    c = dict(PATH_CASES)[name]
    qd, qL, qR, h = rr.path_from_traj(c["traj"], c["dt"], c["J"])
    Md, D = qd.shape
    cap = rr.rate_caps(qd, c["vel"])
    seen = set()
    for R in sorted({0, 1, min(D, 8), 8}):          # n = 2 D + 2 R + 1 rows: fewer pairs than lanes up to 53 rows
        rows = dr.random_affine(np.random.default_rng(1000 * R + Md), Md, R)
        for kw in (dict(), dict(rate_end=0.125), dict(rate_start=0.25, rate_end=0.25), dict(rate_start=MAX_RATE * 1.01)):
            kw = dict(dict(max_rate=MAX_RATE), **kw)
            host = shim.retime_affine(qd, qL, qR, cap, c["acc"], *rows, h, **kw)
            dev = engine.retime_path_affine(qd, qL, qR, cap, c["acc"], *rows, h, **kw)
            host["status"] = np.int32(host["status"])
            _same_bits({k: dev[k][0] for k in PROFILE}, host, PROFILE, what=(name, R, kw))
            seen.add(int(host["status"]))
        if R == 0:                                   # no affine row: the bits of gpmp2mi_retime_path
            plain = engine.retime_path(qd, qL, qR, cap, c["acc"], h, max_rate=MAX_RATE)
            dev = engine.retime_path_affine(qd, qL, qR, cap, c["acc"], None, None, None, None, None, h, max_rate=MAX_RATE)
            _same_bits(dev, plain, ("sdot", "u", "stamps", "duration", "status"), what=(name, "R = 0"))
            assert np.array_equal(_bits(dev["achieved"][:, :4]), _bits(plain["achieved"]))
    assert seen >= {dr.OK, dr.BOUNDARY}


def test_retime_path_affine_rows_do_not_see_each_other(engine):
    """six rows of one shape: fine, STATIC, EMPTY, INVALID, BOUNDARY, fine.  Every row has the bits of the host rule and
    of the same row alone"""
    rng = np.random.default_rng(5)
    N, D, J, dt, R = 6, 7, 2, 0.5, 7
    vel, acc = np.full(D, 1.0), np.full(D, 2.0)
    paths = [rr.path_from_traj(rr.random_traj(rng, N, D, dt, rest=True, pause=b == 5), dt, J) for b in range(6)]
    h, Md = paths[0][3], paths[0][0].shape[0]
    qd, qL, qR = (np.ascontiguousarray([p[i] for p in paths]) for i in range(3))
    cap = np.ascontiguousarray([rr.rate_caps(p[0], vel) for p in paths])
    cxl, cxr, cu, off, bound = dr.random_affine(rng, Md, R)
    cxl, cxr, cu, off = (np.ascontiguousarray(np.broadcast_to(x, (6, Md, R))) for x in (cxl, cxr, cu, off))
    off[1, 4, 2] = bound[2]                 # row 1: the offset alone takes a bound
    qL[2, -1] = 400.0                       # row 2 ends at rest with an acceleration that the forced end rate breaks
    cu[3, 9, 0] = np.nan                    # row 3: a coefficient is not finite
    cap[4, -1] = 1e-4                       # row 4: the forced end rate lies above the last cap
    kw = dict(max_rate=MAX_RATE, rate_end=0.125)
    dev = engine.retime_path_affine(qd, qL, qR, cap, acc, cxl, cxr, cu, off, bound, h, **kw)
    for b in range(6):
        args = (qd[b], qL[b], qR[b], cap[b], acc, cxl[b], cxr[b], cu[b], off[b], bound, h)
        host = shim.retime_affine(*args, **kw)
        host["status"] = np.int32(host["status"])
        _same_bits({k: dev[k][b] for k in PROFILE}, host, PROFILE, what=b)
        _same_bits(engine.retime_path_affine(*args, **kw), dev, PROFILE, rows=(0, b), what=("alone", b))
    assert list(dev["status"]) == [dr.OK, dr.STATIC, dr.EMPTY, dr.INVALID, dr.BOUNDARY, dr.OK]
    assert np.isinf(dev["duration"][1:5]).all() and np.isnan(dev["sdot"][1:5]).all() and np.isnan(dev["achieved"][1:5]).all()


# ------------------------------------------------------------------------------------------- the four arms of "torque limits"
@pytest.fixture(scope="module")
def arms(engine, oracle):
    made = {}

    def get(name):
        if name not in made:
            model = tq.models()[name]()
            r, table = engine.robot(model), tq.case_table(name)
            made[name] = (model, r, oracle.robot(model), table, _dynamics(engine, r, table))
        return made[name]
    return get


@pytest.fixture(scope="module")
def cases(engine, oracle, arms):
    """every case once: the device's outputs, the float64 reference's coefficients and the truth's, shared by the tests
    below and left unchanged"""
    made = {}

    def get(case):
        if case not in made:
            name, (N, J), B = case
            model, r, ro, table, dyn = arms(name)
            D, dt = model.dof(), tq.case_dt(N)
            traj = tq.case_traj(name, N, B)
            lim = E.MotionLimits(D, vel=VEL)
            dev = engine.retime_dynamic_traj(r, dyn, lim, dt, J, traj, max_rate=MAX_RATE)
            made[case] = dict(traj=traj, dt=dt, J=J, D=D, lim=lim, dev=dev,
                              coef=dr.coefficients(oracle, model, table, dt, J, traj),
                              truth=dr.coefficients(oracle, model, table, dt, J, traj, np.longdouble))
        return made[case]
    return get


@pytest.mark.parametrize("case", tq.GPU_CASES, ids=[tq.case_id(c) for c in tq.GPU_CASES])
def test_coefficients_match_the_truth(cases, case):
    c = cases(case)
    assert scoring.checked_states(*case[1]) in (13, 63, 64, 65)
    dev, exp, truth = c["dev"]["coef"], c["coef"], c["truth"]
    for i, what in enumerate(dr.COEF):
        e_gpu, e_cpu = tq.err(dev[:, :, i], truth[:, :, i]), tq.err(exp[:, :, i], truth[:, :, i])
        print(f"{tq.case_id(case)} {what}: e_gpu {e_gpu.max():.2e}, e_cpu {e_cpu.max():.2e}, ratio "
              f"{(e_gpu / np.maximum(e_cpu, FLOOR)).max():.2f}")
        assert (e_gpu <= np.minimum(K * np.maximum(e_cpu, FLOOR), CAP)).all(), (what, e_gpu.max(), e_cpu.max())
    # one-sided states carry their side twice; inside an interval the two sides agree
    N, J = case[1]
    one_sided = np.ones(dev.shape[1], dtype=bool)
    one_sided[np.arange(1, N) * (J + 1)] = False
    assert np.array_equal(_bits(dev[:, one_sided, 1]), _bits(dev[:, one_sided, 2]))


@pytest.mark.parametrize("NJ", tq.SHAPES, ids=lambda x: f"N{x[0]}J{x[1]}")
def test_p_is_exactly_zero_where_the_path_derivative_is(engine, arms, NJ):
    """where q'_k == 0 exactly, p_k == 0 exactly (and m, where q'' == 0 as well): the rule branches on cu == 0.  The
    velocity of a support state is copied, so it is exactly what the row says; between support states the interpolated
    velocity of a row at rest is a rounding error, not 0 (tests/test_gpu_torque.py says why), and is not looked at."""
    N, J = NJ
    model, r, _, table, dyn = arms("wam")
    dt = tq.case_dt(N)
    rows = tq.constructed_rows(N, dt, 1.0)[:3]
    ends = tq.case_traj("wam", N, 3)
    ends[:, 0, 7:] = 0.0                       # rows at rest at both ends
    ends[:, -1, 7:] = 0.0
    lim = E.MotionLimits(7, vel=VEL)
    sup = np.arange(N + 1) * (J + 1)
    for traj in (rows, ends):
        out = engine.retime_dynamic_traj(r, dyn, lim, dt, J, traj, max_rate=MAX_RATE)
        coef = out["coef"][:, sup]                                          # [B][N+1][4][D]
        rest = ~traj[:, :, 7:].any(axis=2)                                  # q' == 0 at this support state
        assert rest.any() and (coef[rest][:, 0] == 0).all(), "p at a state with q' == 0"
        assert (coef[~rest][:, 0] != 0).any()
    out = engine.retime_dynamic_traj(r, dyn, lim, dt, J, rows[:1], max_rate=MAX_RATE)
    coef = out["coef"][0, sup]
    assert out["status"][0] == dr.OK
    assert (coef[:, :3] == 0).all() and (coef[:, 3] != 0).all()             # at rest: nothing but gravity
    if J == 0:      # every stage's rows cap x or bound nothing, and nothing caps: the row runs at max_rate
        assert (out["sdot"] == MAX_RATE).all() and np.array_equal(out["tau_retimed"][0], out["coef"][0, :, 3])
        assert out["achieved"][0, 4] == out["achieved"][0, 5] > 0


@pytest.fixture(scope="module")
def clause_count():
    count = dict(rows=0, second=0)
    yield count
    print("rows compared", count["rows"], "of which the sensitivity clause was needed for", count["second"])


def _reference(c, table, traj, coef, **kw):
    return [dr.retime_dynamic_traj(traj[b], coef[b], dr.torque_limits(table, c["D"]), c["dt"], c["J"], vel=np.full(c["D"], VEL),
                                   max_rate=MAX_RATE, **kw) for b in range(traj.shape[0])]


@pytest.mark.parametrize("case", tq.GPU_CASES, ids=[tq.case_id(c) for c in tq.GPU_CASES])
def test_retime_dynamic_traj_matches_the_numpy_rule(engine, oracle, arms, cases, clause_count, case):
    name, (N, J), B = case
    model, r, ro, table, dyn = arms(name)
    c = cases(case)
    traj, dev, D, dt = c["traj"], c["dev"], c["D"], c["dt"]
    refs = _reference(c, table, traj, c["coef"])
    bent = rr.ulp_perturbed(traj, np.random.default_rng(3))
    moved = _reference(c, table, bent, dr.coefficients(oracle, model, table, dt, J, bent))
    second = 0
    for b in range(B):
        assert dev["status"][b] == refs[b]["status"] == dr.OK, (b, dev["status"][b], refs[b]["status"])
        needs = False
        for k in ("sdot", "stamps", "duration"):
            x, y, z = np.asarray(dev[k][b]), np.asarray(refs[b][k]), np.asarray(moved[b][k])
            e, rel, sens = np.abs(x - y), 1e-12 * np.abs(y), 10.0 * np.abs(z - y)
            print(f"{tq.case_id(case)} row {b} {k}: err {e.max():.2e}, err / 1e-12 rel {np.max(e / np.maximum(rel, 1e-300)):.2e}")
            assert (e <= np.maximum(rel, sens)).all(), (b, k, e.max(), rel.max(), sens.max())
            needs = needs or bool((e > rel).any())
        second += needs
    clause_count["rows"] += B
    clause_count["second"] += second
    # a row alone, and at the end of another batch: the same bits
    b = B // 2
    _same_bits(engine.retime_dynamic_traj(r, dyn, c["lim"], dt, J, traj[b], max_rate=MAX_RATE), dev, NAMES, rows=(0, b),
               what="alone")
    shuffled = np.concatenate([traj[b + 1:], traj[:b + 1], traj[b:b + 1]])
    _same_bits(engine.retime_dynamic_traj(r, dyn, c["lim"], dt, J, shuffled, max_rate=MAX_RATE), dev, NAMES, rows=(B, b),
               what="shuffled")


def test_no_more_than_one_row_in_twenty_needed_the_sensitivity_clause(clause_count):
    """runs behind the cases above (file order)"""
    assert clause_count["rows"] == sum(c[2] for c in tq.GPU_CASES) == 48
    assert 20 * clause_count["second"] <= clause_count["rows"], clause_count


@pytest.mark.parametrize("case", tq.GPU_CASES, ids=[tq.case_id(c) for c in tq.GPU_CASES])
def test_properties_from_the_devices_own_outputs(engine, arms, cases, case):
    name, (N, J), B = case
    model, r, ro, table, dyn = arms(name)
    c = cases(case)
    traj, dev, D, dt = c["traj"], c["dev"], c["D"], c["dt"]
    L = dr.torque_limits(table, D)
    h = dt / (J + 1)
    score = engine.torque_score_traj(r, dyn, dt, J, traj)
    uniform = []
    for b in range(B):
        coef, x, u = dev["coef"][b], dev["sdot"][b] ** 2, dev["u"][b]
        p, mL, mR, tg = (coef[:, i] for i in range(4))
        # tau_retimed = m x + p u + tau_g, to 1e-12 of the size of its terms (x is sdot^2 here, the device's sdot^2
        # before its square root: one rounding apart, which a relative test of a sum that cancels would not forgive)
        want = dr.tau_retimed(coef, x, u)
        size = np.abs(mR) * x[:, None] + np.abs(p) * np.abs(np.r_[u[:-1], u[-2]])[:, None] + np.abs(tg)
        assert (np.abs(dev["tau_retimed"][b] - want) <= 1e-12 * np.maximum(1.0, size)).all(), b
        # achieved[4] is its largest ratio over the two ends of every stage, and the limits hold
        ach = dr.achieved_affine(mL, mR, p, tg, L, h, x, u)
        np.testing.assert_allclose(dev["achieved"][b, 4:], ach, rtol=1e-12, atol=0)
        assert dev["achieved"][b, 4] <= 1 + 2.0 ** -50, (b, dev["achieved"][b, 4] - 1)
        assert dev["achieved"][b, 5] < 1 and abs(dev["achieved"][b, 5] - score["static_ratio"][b]) <= 1e-14
        ends = np.concatenate(dr.affine_values(mL, mR, p, tg, h, x, u))
        assert (np.abs(ends) <= L * (1 + 1e-12)).all(), b
        assert dev["achieved"][b, 0] <= 1 + 1e-9 and (dev["sdot"][b] <= MAX_RATE).all()
        assert dev["duration"][b] == dev["stamps"][b, -1] and dev["stamps"][b, 0] == 0 and (np.diff(dev["stamps"][b]) > 0).all()
        # never slower than the uniform stretch that meets the same limits
        qd = rr.path_from_traj(traj[b], dt, J)[0]
        stretch = max(float(score["torque_time_scale"][b]), float(np.abs(qd).max() / VEL), 1.0 / MAX_RATE)
        assert dev["duration"][b] <= stretch * tq.DURATION * (1 + 1e-12), (b, dev["duration"][b], stretch * tq.DURATION)
        uniform.append(stretch * tq.DURATION)
    print(tq.case_id(case), "re-timed / uniform stretch", np.round(dev["duration"] / np.array(uniform), 4))
    # the torques at planned timing: x = 1, u = 0
    planned = dev["coef"][:, :, 2] + dev["coef"][:, :, 3]
    assert np.abs(planned - score["tau"]).max() <= 1e-11 * max(1.0, np.abs(score["tau"]).max())


@pytest.mark.parametrize("case", [c for c in tq.GPU_CASES if c[0] in ("one", "arm8")], ids=tq.case_id)
def test_without_torque_limits_it_is_re_timing_bit_for_bit(engine, arms, case):
    name, (N, J), B = case
    model, r, ro, table, _ = arms(name)
    D, dt = model.dof(), tq.case_dt(N)
    free = _dynamics(engine, r, dict(table, torque=None))
    traj = tq.case_traj(name, N, B)
    lim = E.MotionLimits(D, vel=VEL, acc=25.0, point_speed=2.0)
    for kw in (dict(max_rate=MAX_RATE), dict(max_rate=2.0, rate_start=0.5, rate_end=0.25)):
        plain = engine.retime_traj(r, lim, dt, J, traj, **kw)
        dyn = engine.retime_dynamic_traj(r, free, lim, dt, J, traj, **kw)
        _same_bits(dyn, plain, ("sdot", "u", "stamps", "duration", "status", "dense_retimed"), what=kw)
        assert np.array_equal(_bits(dyn["achieved"][:, :4]), _bits(plain["achieved"]))
        assert (dyn["achieved"][:, 4:] == 0).all() and (plain["status"] == dr.OK).all()


def test_static_and_invalid_rows(engine, arms):
    model, r, _, table, dyn = arms("wam")
    N, J = 9, 6
    dt = tq.case_dt(N)
    lim = E.MotionLimits(7, vel=VEL)
    traj = tq.case_traj("wam", N, 5)
    clean = engine.retime_dynamic_traj(r, dyn, lim, dt, J, traj, max_rate=MAX_RATE)
    bad = traj.copy()
    bad[1, 3, 2] = np.nan
    bad[3, 5, 7 + 4] = np.inf
    dev = engine.retime_dynamic_traj(r, dyn, lim, dt, J, bad, max_rate=MAX_RATE)
    assert list(dev["status"]) == [0, dr.INVALID, 0, dr.INVALID, 0]
    assert np.isinf(dev["duration"][[1, 3]]).all() and np.isnan(dev["sdot"][[1, 3]]).all()
    assert np.isnan(dev["achieved"][[1, 3]]).all() and np.isnan(dev["tau_retimed"][[1, 3]]).all()
    _same_bits(dev, clean, NAMES, rows=([0, 2, 4], [0, 2, 4]), what="rows beside a NaN row")
    # a joint whose limit gravity alone exceeds: no timing helps
    weak = table["torque"].copy()
    weak[1] = 0.5 * np.abs(clean["coef"][:, :, 3, 1]).max()
    out = engine.retime_dynamic_traj(r, _dynamics(engine, r, dict(table, torque=weak)), lim, dt, J, traj, max_rate=MAX_RATE)
    assert (out["status"] == dr.STATIC).all() and np.isinf(out["duration"]).all() and np.isnan(out["stamps"]).all()
    assert np.isnan(out["dense_retimed"][:, :, 7:]).all() and np.isfinite(out["dense_retimed"][:, :, :7]).all()
    assert np.array_equal(_bits(out["coef"]), _bits(clean["coef"]))          # the coefficients do not depend on the limits


# ------------------------------------------------------------------------------------------------------------ the plan
def _args(p):
    return p.start_conf, p.start_vel, p.end_conf, p.end_vel


@pytest.fixture(scope="module")
def wam16(engine):
    """the 16-row WAM input of the scoring tests solved on the device, with an illustrative inertial table"""
    p, J = ref.motivation_inputs()[0]
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pl = engine.plan(r, s, p.setting, p.B)
    pl.set_problem(*_args(p), p.init)
    pl.optimize()
    t = tables.illustrative_wam()
    t["gravity"] = np.array([0.0, 0.0, -9.81])
    return dict(p=p, J=J, r=r, s=s, pl=pl, res=pl.result(), dt=ref.delta_t(p.setting), table=t,
                dyn=_dynamics(engine, r, t), free=_dynamics(engine, r, dict(t, torque=None)),
                lim=E.MotionLimits(7, **mr.WAM_LIMITS), pairs=engine.generate_self_pairs(r, 2, np.zeros((1, 7))))


def test_plan_form_has_the_bits_of_the_trajectory_form(engine, wam16):
    w = wam16
    pl, r, dyn, lim, dt, J, traj = w["pl"], w["r"], w["dyn"], w["lim"], w["dt"], w["J"], w["res"]["traj"]
    through_plan = pl.retime_dynamic(dyn, lim, J, max_rate=2.0)
    print("status", through_plan["status"], "duration", through_plan["duration"])
    assert (through_plan["status"] == dr.OK).any()
    batch = engine.retime_dynamic_traj(r, dyn, lim, dt, J, traj, max_rate=2.0)
    _same_bits(through_plan, batch, NAMES, what="Plan.retime_dynamic vs Engine.retime_dynamic_traj on the fetched result")
    _same_bits(through_plan, pl.retime_dynamic(dyn, lim, J, max_rate=2.0), NAMES, what="Plan.retime_dynamic twice in a row")
    _same_bits(engine.retime_dynamic_traj(r, dyn, lim, dt, J, traj[11], max_rate=2.0), batch, NAMES, rows=(0, 11),
               what="alone vs row 11 of 16")
    part = pl.retime_dynamic(dyn, lim, J, max_rate=2.0, out={"duration": np.zeros(16)}, tau=False, coef=False)
    assert part["tau_retimed"] is None and part["coef"] is None
    assert np.array_equal(_bits(part["duration"]), _bits(through_plan["duration"]))
    pl.retime_dynamic(dyn, lim, 7, max_rate=2.0)                      # another inter_step grows the workspace
    _same_bits(through_plan, pl.retime_dynamic(dyn, lim, J, max_rate=2.0), NAMES, what="after the workspace grew")
    # without torque limits: the bits of Plan.retime
    plain, free = pl.retime(lim, J, max_rate=2.0), pl.retime_dynamic(w["free"], lim, J, max_rate=2.0)
    _same_bits(free, plain, ("sdot", "u", "stamps", "duration", "status", "dense_retimed"), what="no torque limit")
    assert np.array_equal(_bits(free["achieved"][:, :4]), _bits(plain["achieved"]))
    ok = through_plan["status"] == dr.OK
    assert (through_plan["duration"][ok] >= plain["duration"][ok]).all()     # more rows: never faster


def test_select_retimed_dynamic_is_the_rule_on_the_devices_own_scores(engine, wam16):
    w = wam16
    pl, pairs, lim, dyn, J, res = w["pl"], w["pairs"], w["lim"], w["dyn"], w["J"], w["res"]
    ob, se, mo = pl.score(J), pl.self_score(pairs, J), pl.motion_score(lim, J)
    rt = pl.retime_dynamic(dyn, lim, J, max_rate=2.0)
    fe, st = res["final_error"], res["status"]
    finite = np.isfinite(rt["coef"]).all(axis=(1, 2, 3))
    dur = np.sort(rt["duration"][np.isfinite(rt["duration"])])
    assert dur.size >= 2

    def rule(req, rir, use_pairs, req_self, rpm, md):
        return scoring.retimed_dynamic_rule(fe, st, ob["min_clearance"], ob["out_of_range"], req, rir,
                                            se["min_self_clearance"] if use_pairs else None,
                                            se["invalid"] if use_pairs else None, req_self, mo["pos_margin"], mo["invalid"],
                                            rpm, retime_status=rt["status"], duration=rt["duration"], max_duration=md,
                                            coef_finite=finite)
    one = next(float(d) for d in dur if rule(-np.inf, False, False, 0.0, -np.inf, float(d))[1] == 1)   # leaves one row
    seen = set()
    for req, rir, use_pairs, req_self, rpm, md in (
            (0.0, False, False, 0.0, -np.inf, np.inf), (0.0, True, True, 0.0, -np.inf, np.inf),
            (0.0, False, False, 0.0, -np.inf, float(np.median(dur))), (-np.inf, False, True, -np.inf, -0.1, float(np.median(dur))),
            (0.0, False, False, 0.0, 0.0, np.inf), (-np.inf, False, False, 0.0, -np.inf, float(dur[0]) * 0.99),
            (-np.inf, False, False, 0.0, -np.inf, one)):                 # the last two: no row, then one row
        want = rule(req, rir, use_pairs, req_self, rpm, md)
        got = pl.select_retimed_dynamic(J, lim, dyn, rpm, md, 2.0, None, None, req, rir, pairs if use_pairs else None, req_self)
        print((req, rir, use_pairs, req_self, rpm, md), "->", got["best"], got["n_eligible"], got["duration_best"])
        assert (got["best"], got["n_eligible"]) == want, (req, rir, use_pairs, req_self, rpm, md, want)
        seen.add(want)
        if want[0] >= 0:
            b = want[0]
            assert got["duration_best"] == rt["duration"][b]
            assert np.array_equal(_bits(got["stamps_best"]), _bits(rt["stamps"][b]))
            assert np.array_equal(_bits(got["tau_best"]), _bits(rt["tau_retimed"][b]))
            assert np.array_equal(_bits(got["traj_best"]), _bits(res["traj"][b]))
            assert np.array_equal(_bits(got["dense_best"]), _bits(rt["dense_retimed"][b]))
        else:
            assert got["duration_best"] is None and got["stamps_best"] is None and got["tau_best"] is None
    assert len(seen) >= 3 and (-1, 0) in seen and any(n == 1 for _, n in seen)
    # without torque limits: the row select_retimed chooses
    a = pl.select_retimed(J, lim, -np.inf, np.inf, 2.0)
    b = pl.select_retimed_dynamic(J, lim, w["free"], -np.inf, np.inf, 2.0)
    assert (a["best"], a["n_eligible"]) == (b["best"], b["n_eligible"]) and a["best"] >= 0
    assert a["duration_best"] == b["duration_best"] and np.array_equal(_bits(a["dense_best"]), _bits(b["dense_best"]))


def test_the_existing_calls_are_left_alone(engine, wam16):
    w = wam16
    pl, lim, dyn, J, pairs = w["pl"], w["lim"], w["dyn"], w["J"], w["pairs"]
    before = pl.retime(lim, J, max_rate=2.0), pl.torque_score(dyn, J), pl.select(J)
    pl.retime_dynamic(dyn, lim, J, max_rate=2.0)
    pl.select_retimed_dynamic(J, lim, dyn, -np.inf, np.inf, 2.0, None, None, 0.0, False, pairs, 0.0)
    after = pl.retime(lim, J, max_rate=2.0), pl.torque_score(dyn, J), pl.select(J)
    _same_bits(before[0], after[0], scoring.RETIME_NAMES, what="plan_retime around the new calls")
    _same_bits(before[1], after[1], scoring.TORQUE_NAMES, what="plan_torque_score around the new calls")
    assert (before[2]["best"], before[2]["n_eligible"]) == (after[2]["best"], after[2]["n_eligible"])
    assert np.array_equal(_bits(before[2]["dense_best"]), _bits(after[2]["dense_best"]))


def test_refusals_with_live_handles(engine, wam16, arms):
    w = wam16
    pl, r, dyn, lim, J, p = w["pl"], w["r"], w["dyn"], w["lim"], w["J"], w["p"]
    _, r8, _, _, dyn8 = arms("arm8")
    _, _, _, _, dyn_tilted = arms("wam")          # the same joints behind another base pose and other biases
    for other in (dyn8, dyn_tilted):
        for call in (lambda: pl.retime_dynamic(other, lim, J), lambda: pl.select_retimed_dynamic(J, lim, other),
                     lambda: engine.retime_dynamic_traj(r, other, lim, 0.1, 1, np.zeros((1, 3, 14)))):
            with pytest.raises(E.Gpmp2miError) as ei:
                call()
            assert ei.value.code == 1 and "another robot" in str(ei.value)
    import gpmp2_amd as g
    mobile = engine.robot(g.generateMobileArm("SimpleTwoLinksArm"))
    out = np.full((1, 3), 7.0)
    lib = engine.lib
    rc = lib.gpmp2mi_retime_dynamic_traj(mobile.ptr, dyn.ptr, lim.ref(7), 0.1, 0, 1, 2, E.dptr(np.zeros((1, 3, 10))), 1.0, -1.0,
                                         -1.0, E.dptr(out), *([None] * 8))
    assert rc == 4 and b"fixed-base" in lib.gpmp2mi_last_error() and (out == 7.0).all()
    bad = _capi.MotionLimitsC(None, None, E.dptr(np.zeros(7)), None, np.inf)
    assert lib.gpmp2mi_plan_retime_dynamic(pl.h.ptr, dyn.ptr, C.byref(bad), J, 1.0, -1.0, -1.0, *([None] * 9)) == 1
    assert lib.gpmp2mi_plan_retime_dynamic(pl.h.ptr, dyn.ptr, lim.ref(7), -1, 1.0, -1.0, -1.0, *([None] * 9)) == 1
    assert lib.gpmp2mi_plan_retime_dynamic(pl.h.ptr, dyn.ptr, lim.ref(7), J, 1.0, -1.0, -1.0, *([None] * 9)) == 0   # all NULL
    assert lib.gpmp2mi_plan_select_retimed_dynamic(pl.h.ptr, J, 0.0, 0, None, 0.0, lim.ref(7), 0.0, 1.0, -1.0, -1.0, np.inf,
                                                   dyn.ptr, *([None] * 7)) == 0
    fresh = engine.plan(r, w["s"], p.setting, p.B)
    for call in (lambda: fresh.retime_dynamic(dyn, lim, J), lambda: fresh.select_retimed_dynamic(J, lim, dyn)):
        with pytest.raises(E.Gpmp2miError) as ei:
            call()
        assert ei.value.code == 1 and "not been optimized" in str(ei.value)
    fresh.close()
    assert (pl.retime_dynamic(dyn, lim, J, max_rate=2.0)["status"] != dr.INVALID).all()      # the plan is as usable as before


# ------------------------------------------------------------------------------------------------------ the `_dev` forms
class _DevBuf:
    """a device buffer through the HIP runtime (ctypes), for the device-pointer entry points"""
    hip = None

    def __init__(self, a):
        if _DevBuf.hip is None:
            _DevBuf.hip = C.CDLL("libamdhip64.so")
        self.a = np.ascontiguousarray(a)
        self.ptr = C.c_void_p()
        assert _DevBuf.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(max(self.a.nbytes, 8))) == 0
        assert _DevBuf.hip.hipMemcpy(self.ptr, self.a.ctypes.data_as(C.c_void_p), C.c_size_t(self.a.nbytes), 1) == 0

    def get(self):
        out = np.empty_like(self.a)
        assert _DevBuf.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.ptr, C.c_size_t(self.a.nbytes), 2) == 0
        return out

    def __del__(self):
        if self.ptr:
            _DevBuf.hip.hipFree(self.ptr)


def test_dev_forms_equal_the_host_calls_bit_for_bit(engine, wam16):
    """device buffers on the null stream; hipMemcpy back waits for it"""
    w = wam16
    pl, r, pairs, lim, dyn, J, dt = w["pl"], w["r"], w["pairs"], w["lim"], w["dyn"], w["J"], w["dt"]
    B, N, D = 16, 12, 7
    Md = scoring.checked_states(N, J)
    host = pl.retime_dynamic(dyn, lim, J, max_rate=2.0)
    shapes = dict(sdot=(B, Md), u=(B, Md), stamps=(B, Md), duration=(B,), status=(B,), achieved=(B, 6),
                  dense_retimed=(B, Md, 2 * D), tau_retimed=(B, Md, D), coef=(B, Md, 4, D))
    assert tuple(shapes) == NAMES

    def outs():
        return {k: _DevBuf(np.full(s, -7, dtype=np.int32) if k == "status" else np.full(s, np.nan)) for k, s in shapes.items()}
    o = outs()
    pl.retime_dynamic_dev(dyn, lim, J, max_rate=2.0, **{k: v.ptr.value for k, v in o.items()})
    _same_bits({k: v.get() for k, v in o.items()}, host, shapes, what="Plan.retime_dynamic_dev")
    o = outs()
    traj = _DevBuf(w["res"]["traj"])
    rc = engine.lib.gpmp2mi_retime_dynamic_traj_dev(r.ptr, dyn.ptr, lim.ref(7), dt, J, B, N, traj.ptr, 2.0, -1.0, -1.0,
                                                    *[o[k].ptr for k in shapes], None)
    assert rc == 0
    _same_bits({k: v.get() for k, v in o.items()}, host, shapes, what="gpmp2mi_retime_dynamic_traj_dev")
    part = _DevBuf(np.full(B, np.nan))                   # any output may be NULL
    pl.retime_dynamic_dev(dyn, lim, J, max_rate=2.0, duration=part.ptr.value)
    assert np.array_equal(_bits(part.get()), _bits(host["duration"]))
    dur = np.sort(host["duration"][np.isfinite(host["duration"])])
    md = float(dur[min(3, dur.size - 1)])
    sel = pl.select_retimed_dynamic(J, lim, dyn, -np.inf, md, 2.0, None, None, 0.0, False, pairs, -np.inf)
    assert sel["best"] >= 0
    best, n = _DevBuf(np.full(1, -7, dtype=np.int32)), _DevBuf(np.full(1, -7, dtype=np.int32))
    db_, sb, tau = _DevBuf(np.full(1, np.nan)), _DevBuf(np.full(Md, np.nan)), _DevBuf(np.full((Md, D), np.nan))
    tb, db = _DevBuf(np.full((N + 1, 2 * D), np.nan)), _DevBuf(np.full((Md, 2 * D), np.nan))
    pl.select_retimed_dynamic_dev(J, lim, dyn, -np.inf, md, 2.0, None, None, 0.0, False, pairs, -np.inf, best.ptr.value,
                                  n.ptr.value, db_.ptr.value, sb.ptr.value, tau.ptr.value, tb.ptr.value, db.ptr.value)
    assert (int(best.get()[0]), int(n.get()[0])) == (sel["best"], sel["n_eligible"])
    assert db_.get()[0] == sel["duration_best"]
    for got, name in ((sb, "stamps_best"), (tau, "tau_best"), (tb, "traj_best"), (db, "dense_best")):
        assert np.array_equal(_bits(got.get()), _bits(sel[name])), name
    # a bound no row meets leaves the outputs about the chosen row alone; `best` may be NULL
    pl.select_retimed_dynamic_dev(J, lim, dyn, -np.inf, 1e-3, 2.0, n_eligible=n.ptr.value, duration_best=db_.ptr.value,
                                  tau_best=tau.ptr.value)
    assert int(n.get()[0]) == 0 and db_.get()[0] == sel["duration_best"]
    assert np.array_equal(_bits(tau.get()), _bits(sel["tau_best"]))
    # the bare rule with device pointers
    c = dict(PATH_CASES)["long-D3N20J4"]
    qd, qL, qR, h = rr.path_from_traj(c["traj"], c["dt"], c["J"])
    cap = rr.rate_caps(qd, c["vel"])
    M, R = qd.shape[0], 5
    rows = dr.random_affine(np.random.default_rng(9), M, R)
    want = engine.retime_path_affine(qd, qL, qR, cap, c["acc"], *rows, h, max_rate=MAX_RATE)
    ins = [_DevBuf(x) for x in (qd, qL, qR, cap)]
    aff = [_DevBuf(x) for x in rows[:4]]
    po = dict(sdot=_DevBuf(np.zeros(M)), u=_DevBuf(np.zeros(M)), stamps=_DevBuf(np.zeros(M)), duration=_DevBuf(np.zeros(1)),
              status=_DevBuf(np.full(1, -7, dtype=np.int32)), achieved=_DevBuf(np.zeros(6)))
    ws = _DevBuf(np.zeros(M * (3 + 4 * (2 * 3 + 2 * R))))
    rc = engine.lib.gpmp2mi_retime_path_affine_dev(1, M, 3, *[x.ptr for x in ins], E.dptr(np.ascontiguousarray(c["acc"])), R,
                                                   *[x.ptr for x in aff], E.dptr(rows[4]), h, MAX_RATE, -1.0, -1.0,
                                                   *[po[k].ptr for k in PROFILE], ws.ptr, None)
    assert rc == 0
    _same_bits({k: v.get().reshape(want[k].shape) for k, v in po.items()}, want, PROFILE, what="gpmp2mi_retime_path_affine_dev")
