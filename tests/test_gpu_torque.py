"""The torque limits on the device (include/gpmp2mi.h "torque limits") against the link-frame two-pass reference of
tests/torque_reference.py, through every entry point: caller buffers and plans; values at the tile edge on both sides
and for four arms, constructed rows with known answers, determinism, selection, and that the existing calls are left
alone.

Tolerance (DESIGN.md "torque limits", scripts/torque_error.py -> profiles/torque_error.txt): with
err(x, truth) = |x - truth| / max(1, |truth|), every value is within K * max(e_cpu, FLOOR) and within CAP of a truth in
np.longdouble, where e_cpu is the float64 reference's own error against that truth (tr.K, tr.FLOOR = 2^-52,
tr.CAP = 1e-11).  `worst` is compared wherever the reference's gap to the runner-up is 0 or above
2 CAP max(1, |value|); tests/test_torque_cpu.py asserts that the inputs leave at most one row in eight undecided."""
import ctypes as C

import numpy as np
import pytest

import motion_reference as mr
import score_reference as ref
import torque_reference as tr
from gpmp2_amd import _capi, scoring
from gpmp2_amd import dynamics as tables
from gpmp2_amd import engine as E

pytestmark = pytest.mark.gpu
NAMES = scoring.TORQUE_NAMES


def _same_bits(a, b, rows=None, what="", names=NAMES):
    for k in names:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows[0]], b[k][rows[1]])
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.dtype == np.float64:
            x, y = x.view(np.int64), y.view(np.int64)
        assert np.array_equal(x, y), (what, k)


def _dynamics(engine, r, table):
    return engine.dynamics(r, table["mass"], table["com"], table["inertia"], table["gravity"], table.get("torque"))


def _check_against_reference(dev, exp, truth, label):
    for k in tr.VALUES + ("tau",):
        e_gpu, e_cpu = tr.err(dev[k], truth[k]), tr.err(exp[k], truth[k])
        bound = np.minimum(tr.K * np.maximum(e_cpu, tr.FLOOR), tr.CAP)
        print(f"{label} {k}: e_gpu {e_gpu.max():.2e}, e_cpu {e_cpu.max():.2e}, ratio "
              f"{(e_gpu / np.maximum(e_cpu, tr.FLOOR)).max():.2f}")
        assert (e_gpu <= bound).all(), (label, k, e_gpu.max(), e_cpu.max())
    assert np.array_equal(dev["invalid"], exp["invalid"]), (label, dev["invalid"], exp["invalid"])
    for c, kind in enumerate(tr.KINDS):
        decided = tr.decided(exp, c)
        differs = (dev["worst"][:, c] != exp["worst"][:, c]).any(axis=1)
        assert not (differs & decided).any(), (label, kind, dev["worst"][differs, c], exp["worst"][differs, c])


@pytest.fixture(scope="module")
def arms(engine, oracle):
    made = {}

    def get(name):
        if name not in made:
            model = tr.models()[name]()
            r, table = engine.robot(model), tr.case_table(name)
            made[name] = (model, r, oracle.robot(model), table, _dynamics(engine, r, table))
        return made[name]
    return get


@pytest.mark.parametrize("case", tr.GPU_CASES, ids=[tr.case_id(c) for c in tr.GPU_CASES])
def test_scores_match_the_reference(engine, oracle, arms, case):
    name, (N, J), B = case
    model, r, ro, table, dyn = arms(name)
    D, dt = model.dof(), tr.case_dt(N)
    traj = tr.case_traj(name, N, B)
    assert scoring.checked_states(N, J) in (13, 63, 64, 65)
    exp = tr.reference_torque_score(oracle, model, table, dt, J, traj)
    truth = tr.truth_torque_score(oracle, model, table, dt, J, traj)
    dev = engine.torque_score_traj(r, dyn, dt, J, traj)
    _check_against_reference(dev, exp, truth, tr.case_id(case))
    if name == "two":   # the torques against the textbook closed form as well
        U, first, _, _ = tr.checked_inputs(oracle, D, dt, J, traj, np.longdouble)
        want = tr.planar_two_link(table, U[:, :, :D], U[:, :, D:], first).reshape(dev["tau"].shape)
        assert tr.err(dev["tau"], want).max() <= tr.CAP
    # a row alone, and at the end of a shuffled batch: the same bits
    b = B // 2
    _same_bits(engine.torque_score_traj(r, dyn, dt, J, traj[b]), dev, rows=(0, b), what="alone vs in its batch")
    shuffled = np.concatenate([traj[b + 1:], traj[:b + 1], traj[b:b + 1]])
    _same_bits(engine.torque_score_traj(r, dyn, dt, J, shuffled), dev, rows=(B, b), what="at the end of another batch")


@pytest.mark.parametrize("NJ", tr.SHAPES, ids=lambda x: f"N{x[0]}J{x[1]}")
def test_constructed_rows_have_their_known_answers(engine, oracle, arms, NJ):
    N, J = NJ
    model, r, ro, table, _ = arms("wam")
    dt = tr.case_dt(N)
    only = np.full(7, np.inf)
    only[tr.PEAK_JOINT] = table["torque"][tr.PEAK_JOINT]
    t_only = dict(table, torque=only)
    d_only = _dynamics(engine, r, t_only)
    rest = np.zeros((1, 2, 14))
    rest[:, :, :7] = tr.REST
    sign = np.sign(engine.torque_score_traj(r, d_only, dt, 0, rest)["tau"][0, 0, tr.PEAK_JOINT])
    rows = tr.constructed_rows(N, dt, sign)
    with np.errstate(invalid="ignore"):
        exp = tr.reference_torque_score(oracle, model, t_only, dt, J, rows)
        truth = tr.truth_torque_score(oracle, model, t_only, dt, J, rows)
    dev = engine.torque_score_traj(r, d_only, dt, J, rows)
    m, j, L = tr.PEAK_STATE * (J + 1), tr.PEAK_JOINT, only[tr.PEAK_JOINT]
    for k in tr.VALUES:
        e_gpu, e_cpu = tr.err(dev[k], truth[k]), tr.err(exp[k], truth[k])
        assert (e_gpu <= np.minimum(tr.K * np.maximum(e_cpu, tr.FLOOR), tr.CAP)).all(), (k, dev[k], exp[k])
    # At rest: nothing but gravity, and no stretch is needed.  With J = 0 every checked state is a copy and the motion
    # part is 0 exactly.  With J > 0 the interpolated velocity of k_interpolate_traj's expressions is l21 q + p21 q with
    # l21 = -p21, which a fused multiply-add leaves at the rounding error of one product (about 1e-16) instead of 0; the
    # motion part is quadratic in it (about 1e-30, far below an ulp of the gravity torque), and its square root passed
    # the value check above against a truth of exactly 0.
    assert dev["torque_ratio"][0] == dev["static_ratio"][0] > 0 and tuple(dev["worst"][0, 0]) == tuple(dev["worst"][0, 1])
    if J == 0:
        assert dev["torque_time_scale"][0] == 0 and tuple(dev["worst"][0, 0]) == (0, j) and tuple(dev["worst"][0, 2]) == (0, j)
    # the only limited joint peaks at the chosen state: on its right side in row 1, on its left side in row 2
    for b in (1, 2):
        assert tuple(dev["worst"][b, 0]) == (m, j) and tuple(dev["worst"][b, 2]) == (m, j)
    assert dev["torque_ratio"][1] == abs(dev["tau"][1, m, j]) / L
    assert dev["torque_ratio"][2] > abs(dev["tau"][2, m, j]) / L
    assert tr.err(dev["torque_ratio"][2], abs(truth["tau_left"][2, m, j]) / L) <= tr.CAP
    # a NaN in one state is counted, and the rows beside it are untouched
    assert np.array_equal(dev["invalid"], exp["invalid"]) and dev["invalid"][3] > 0 and (dev["invalid"][:3] == 0).all()
    assert np.isfinite(dev["torque_ratio"][3]) and abs(dev["static_ratio"][3] - dev["static_ratio"][0]) <= 1e-14
    _same_bits(engine.torque_score_traj(r, d_only, dt, J, rows[:3]), dev, rows=(slice(0, 3), slice(0, 3)), what="beside a NaN row")
    # statically overloaded: no timing helps
    weak = engine.torque_score_traj(r, _dynamics(engine, r, dict(table, torque=np.full(7, 0.01))), dt, J, rows[:1])
    assert weak["static_ratio"][0] >= 1 and np.isposinf(weak["torque_time_scale"][0])
    # without limits nothing is limited, and the torques are the same bits
    free = engine.torque_score_traj(r, _dynamics(engine, r, dict(table, torque=None)), dt, J, rows[:3])
    assert (free["torque_ratio"] == 0).all() and (free["torque_time_scale"] == 0).all() and (free["worst"] == -1).all()
    _same_bits(free, dev, rows=(slice(0, 3), slice(0, 3)), names=("tau",), what="tau does not depend on the limits")


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


def test_a_row_scores_the_same_bits_through_the_plan_and_through_caller_buffers(engine, oracle, wam16):
    w = wam16
    pl, r, dyn, dt, J, traj = w["pl"], w["r"], w["dyn"], w["dt"], w["J"], w["res"]["traj"]
    through_plan = pl.torque_score(dyn, J)
    ro = oracle.robot(w["p"].model)
    exp = tr.reference_torque_score(oracle, w["p"].model, w["table"], dt, J, traj)
    truth = tr.truth_torque_score(oracle, w["p"].model, w["table"], dt, J, traj)
    _check_against_reference(through_plan, exp, truth, "wam16 through the plan")
    batch = engine.torque_score_traj(r, dyn, dt, J, traj)
    _same_bits(through_plan, batch, what="Plan.torque_score vs Engine.torque_score_traj on the fetched result")
    _same_bits(through_plan, pl.torque_score(dyn, J), what="Plan.torque_score twice in a row")
    _same_bits(engine.torque_score_traj(r, dyn, dt, J, traj[11]), batch, rows=(0, 11), what="alone vs row 11 of 16")
    part = pl.torque_score(dyn, J, out={"torque_time_scale": np.zeros(16)}, tau=False)
    assert part["tau"] is None
    assert np.array_equal(part["torque_time_scale"].view(np.int64), through_plan["torque_time_scale"].view(np.int64))
    pl.torque_score(dyn, 9)                              # another inter_step grows the workspace
    _same_bits(through_plan, pl.torque_score(dyn, J), what="after the workspace grew")


def test_select_dynamic_is_the_rule_on_the_devices_own_scores(engine, wam16):
    w = wam16
    pl, pairs, lim, dyn, J, res = w["pl"], w["pairs"], w["lim"], w["dyn"], w["J"], w["res"]
    ob, se, mo, to = pl.score(J), pl.self_score(pairs, J), pl.motion_score(lim, J), pl.torque_score(dyn, J)
    fe, st = res["final_error"], res["status"]
    both = np.maximum(mo["time_scale"], to["torque_time_scale"])
    finite = np.sort(both[np.isfinite(both)])
    seen = set()
    for req, rir, use_pairs, rpm, mts in ((0.0, False, False, -np.inf, np.inf), (0.0, True, True, -np.inf, np.inf),
                                          (-np.inf, False, False, -np.inf, float(finite[len(finite) // 2])),
                                          (-np.inf, False, True, -np.inf, float(finite[0])),
                                          (0.0, False, False, -np.inf, 1e-3)):
        want = scoring.dynamic_rule(fe, st, ob["min_clearance"], ob["out_of_range"], req, rir,
                                    se["min_self_clearance"] if use_pairs else None, se["invalid"] if use_pairs else None,
                                    0.0, mo["pos_margin"], mo["time_scale"], mo["invalid"], rpm, mts,
                                    to["torque_time_scale"], to["invalid"])
        got = pl.select_dynamic(J, lim, dyn, rpm, mts, req, rir, pairs if use_pairs else None, 0.0)
        print((req, rir, use_pairs, rpm, mts), "->", got["best"], got["n_eligible"], got["time_scale_best"])
        assert (got["best"], got["n_eligible"]) == want, (req, rir, use_pairs, rpm, mts, want)
        seen.add(want)
        if want[0] >= 0:
            assert got["time_scale_best"] == both[want[0]]
            assert np.array_equal(got["tau_best"].view(np.int64), to["tau"][want[0]].view(np.int64))
            assert np.array_equal(got["traj_best"].view(np.int64), res["traj"][want[0]].view(np.int64))
        else:
            assert got["time_scale_best"] is None and got["tau_best"] is None and got["traj_best"] is None
    assert len(seen) >= 2 and (-1, 0) in seen          # the thresholds told rows apart, and one refused them all
    # with torque limits of +inf: the row select_feasible chooses
    for rpm, mts in ((-np.inf, np.inf), (-np.inf, float(np.median(mo["time_scale"])))):
        a, b = pl.select_feasible(J, lim, rpm, mts), pl.select_dynamic(J, lim, w["free"], rpm, mts)
        assert (a["best"], a["n_eligible"]) == (b["best"], b["n_eligible"])
        if a["best"] >= 0:
            assert a["time_scale_best"] == b["time_scale_best"] and np.array_equal(a["dense_best"], b["dense_best"])


def test_the_existing_calls_are_left_alone(engine, wam16):
    w = wam16
    pl, lim, dyn, J, pairs = w["pl"], w["lim"], w["dyn"], w["J"], w["pairs"]
    before_m, before_r = pl.motion_score(lim, J), pl.retime(lim, J)
    pl.torque_score(dyn, J)
    pl.select_dynamic(J, lim, dyn, -np.inf, np.inf, 0.0, False, pairs, 0.0)
    after_m, after_r = pl.motion_score(lim, J), pl.retime(lim, J)
    _same_bits(before_m, after_m, names=scoring.MOTION_NAMES, what="plan_motion_score around a torque call")
    _same_bits(before_r, after_r, names=scoring.RETIME_NAMES, what="plan_retime around a torque call")


def test_refusals_with_live_handles(engine, wam16, arms):
    w = wam16
    pl, r, dyn, J, t = w["pl"], w["r"], w["dyn"], w["J"], w["table"]
    _, r8, _, _, dyn8 = arms("arm8")
    _, _, _, _, dyn_tilted = arms("wam")          # the same joints behind another base pose and other biases
    for other in (dyn8, dyn_tilted):
        with pytest.raises(E.Gpmp2miError) as ei:
            pl.torque_score(other, J)
        assert ei.value.code == 1 and "another robot" in str(ei.value)
        with pytest.raises(E.Gpmp2miError) as ei:
            engine.torque_score_traj(r, other, 0.1, 1, np.zeros((1, 3, 14)))
        assert ei.value.code == 1 and "another robot" in str(ei.value)
    with pytest.raises(E.Gpmp2miError) as ei:
        pl.select_dynamic(J, w["lim"], dyn8)
    assert ei.value.code == 1
    assert pl.torque_score(dyn, J)["invalid"].sum() == 0                       # the plan is as usable as before
    # the description, checked against a live robot before any device work
    lib, out = engine.lib, C.c_void_p()

    def create(robot=r, gravity=(0.0, 0.0, -9.81), **kw):
        a = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in dict(t, **kw).items() if k != "gravity" and v is not None}
        desc = _capi.DynamicsDescC(E.dptr(a["mass"]), E.dptr(a["com"]), E.dptr(a["inertia"]), (C.c_double * 3)(*gravity),
                                   E.dptr(a.get("torque")))
        return lib.gpmp2mi_dynamics_create(robot.ptr, C.byref(desc), C.byref(out))
    at = lambda x, i, v: np.where(np.arange(np.size(x)).reshape(np.shape(x)) == i, v, x)
    assert create(mass=at(t["mass"], 2, -1.0)) == 1 and create(mass=at(t["mass"], 0, np.nan)) == 1
    assert create(com=at(t["com"], 5, np.inf)) == 1 and create(inertia=at(t["inertia"], 7, -1e-3)) == 1
    assert create(inertia=at(t["inertia"], 4, np.nan)) == 1 and create(gravity=(0.0, np.nan, 0.0)) == 1
    assert create(torque=at(t["torque"], 3, 0.0)) == 1 and create(torque=at(t["torque"], 3, np.nan)) == 1
    assert out.value is None
    assert create(torque=at(t["torque"], 3, np.inf)) == 0 and out.value is not None    # +inf: no limit for that joint
    lib.gpmp2mi_dynamics_destroy(out)
    lib.gpmp2mi_dynamics_destroy(None)
    import gpmp2_amd as g
    mobile = engine.robot(g.generateMobileArm("SimpleTwoLinksArm"))
    assert create(robot=mobile) == 4 and b"fixed-base" in lib.gpmp2mi_last_error()
