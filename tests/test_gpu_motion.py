"""The motion limits on the device (include/gpmp2mi.h "motion limits") against the CPU oracle's composition
interpolate_traj (both halves) -> sphere_centers (Jacobians) -> numpy (tests/motion_reference.py), through every entry
point: caller buffers and plans; values at every tile edge and every robot kind, constructed rows with known answers,
exact ties, non-finite input, determinism, selection, and that the existing calls are left alone.

Tolerance (DESIGN.md "motion limits", scripts/motion_error.py -> profiles/motion_error.txt): with
err(x, truth) = |x - truth| / max(1, |truth|), every value is within K * max(e_cpu, FLOOR) and within CAP of a truth in
np.longdouble (the Hermite closed form of the GP mean, the Pose2 interpolator with its scalars for the mobile kinds, the
oracle's Jacobians: mr.truth_motion_score), where e_cpu is the float64 reference's own error against that truth.  K = 8, FLOOR = 2^-52, CAP = 1e-12 (mr.K, mr.FLOOR, mr.CAP).
`worst` is compared wherever the reference's gap to the runner-up is 0 (the rule decides) or above 2 CAP max(1, |value|);
tests/test_motion_cpu.py asserts that the inputs leave at most one row in eight undecided (PR2: see mr.SHARE_EXEMPT)."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import motion_reference as mr
import score_reference as ref
import self_reference as sr
from gpmp2_amd import _capi, scoring
from gpmp2_amd import engine as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEVEN = scoring.MOTION_NAMES


def _limits(D, lim):
    return E.MotionLimits(D, **{k: v for k, v in lim.items() if v is not None})


def _same_bits(a, b, rows=None, what="", names=SEVEN):
    for k in names:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows[0]], b[k][rows[1]])
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.dtype == np.float64:
            x, y = x.view(np.int64), y.view(np.int64)
        assert np.array_equal(x, y), (what, k, a[k], b[k])


def _check_against_reference(dev, exp, label, truth, exempt=()):
    """values within the tolerance of the truth, invalid equal, worst equal wherever the reference decides it"""
    for k in mr.VALUES:
        e_gpu, e_cpu = mr.err(dev[k], truth[k]), mr.err(exp[k], truth[k])
        bound = np.minimum(mr.K * np.maximum(e_cpu, mr.FLOOR), mr.CAP)
        print(f"{label} {k}: e_gpu {e_gpu.max():.2e}, e_cpu {e_cpu.max():.2e}, bound {bound.min():.2e}")
        assert (e_gpu <= bound).all(), (label, k, dev[k], exp[k], e_gpu, bound)
    assert np.array_equal(dev["invalid"], exp["invalid"]), (label, dev["invalid"], exp["invalid"])
    for c, kind in enumerate(mr.KINDS):
        decided = mr.decided(exp, c)
        if c in exempt:
            with np.errstate(invalid="ignore"):
                decided &= ~(exp["gap"][:, c] == 0)
        differs = (dev["worst"][:, c] != exp["worst"][:, c]).any(axis=1)
        assert not (differs & decided).any(), (label, kind, dev["worst"][differs, c], exp["worst"][differs, c], exp["gap"][differs, c])


@pytest.fixture(scope="module")
def robots_(engine, oracle):
    made = {}

    def get(name):
        if name not in made:
            model = mr.models()[name]()
            made[name] = (model, engine.robot(model), oracle.robot(model))
        return made[name]
    return get


@pytest.mark.parametrize("case", mr.GPU_CASES, ids=[mr.case_id(c) for c in mr.GPU_CASES])
def test_scores_match_the_reference(engine, oracle, robots_, case):
    name, (N, J), B = case
    model, r, ro = robots_(name)
    D = model.dof()
    lim, dt = mr.case_limits(name), mr.case_dt(name)
    traj = mr.case_traj(name, N, B)
    assert traj.shape == (B, N + 1, 2 * D)
    exp = mr.oracle_motion_score(oracle, model, ro, lim, dt, J, traj)
    truth = mr.truth_motion_score(oracle, model, ro, lim, dt, J, traj)
    dev = engine.motion_score_traj(r, _limits(D, lim), dt, J, traj)
    _check_against_reference(dev, exp, mr.case_id(case), truth, mr.SHARE_EXEMPT.get(name, ()))
    if name == "config5":   # the Pose2 coordinates enter neither the position margin nor the acceleration ratio
        assert (dev["worst"][:, 0, 1] >= 3).all() and (dev["worst"][:, 2, 1] >= 3).all()
        assert (dev["pos_margin"] > -1.0).all() and (dev["acc_ratio"] < 1e3).all()
    # acc_ratio does not depend on inter_step: the same bits with another one
    other = engine.motion_score_traj(r, _limits(D, lim), dt, J + 1, traj)
    _same_bits({"acc_ratio": other["acc_ratio"], "w": other["worst"][:, 2]}, {"acc_ratio": dev["acc_ratio"], "w": dev["worst"][:, 2]},
               names=("acc_ratio", "w"), what="acc_ratio at another inter_step")
    # a row alone, and in another batch at another position: the same bits
    b = B // 2
    _same_bits(engine.motion_score_traj(r, _limits(D, lim), dt, J, traj[b]), dev, rows=(0, b), what="alone vs in its batch")
    shuffled = np.concatenate([traj[b + 1:], traj[:b + 1], traj[b:b + 1]])
    _same_bits(engine.motion_score_traj(r, _limits(D, lim), dt, J, shuffled), dev, rows=(B, b), what="at the end of another batch")


@pytest.mark.parametrize("NJ", [(8, 7), (12, 4), (12, 0)], ids=lambda x: f"N{x[0]}J{x[1]}")
def test_constructed_rows_have_their_extrema_where_they_were_put(engine, oracle, robots_, NJ):
    N, J = NJ
    model, r, ro = robots_("wam")
    S, Md = model.nr_body_spheres(), scoring.checked_states(N, J)
    rows = mr.constructed_rows(N)
    exp = mr.oracle_motion_score(oracle, model, ro, mr.WAM_ROUND, sr.DELTA_T, J, rows)
    dev = engine.motion_score_traj(r, _limits(7, mr.WAM_ROUND), sr.DELTA_T, J, rows)
    truth = mr.truth_motion_score(oracle, model, ro, mr.WAM_ROUND, sr.DELTA_T, J, rows)
    for k in mr.VALUES:
        e_gpu, e_cpu = mr.err(dev[k], truth[k]), mr.err(exp[k], truth[k])
        assert (e_gpu <= np.minimum(mr.K * np.maximum(e_cpu, mr.FLOOR), mr.CAP)).all(), (k, dev[k], exp[k], e_gpu, e_cpu)
    assert np.array_equal(dev["invalid"], exp["invalid"]) and (dev["invalid"] == 0).all()
    assert tuple(dev["worst"][0, 2]) == (0, 2)                         # the first interval, its first end
    assert tuple(dev["worst"][1, 2]) == (2 * (N - 1) + 1, 4)           # the last interval, its last end
    assert tuple(dev["worst"][2, 3]) == (Md - 1, S - 1)                # the last checked state, the last sphere
    if J == 0:      # the constant-velocity line under uniform limits: exact ties, the lowest indices
        assert tuple(dev["worst"][3, 1]) == (0, 0) and tuple(dev["worst"][3, 2]) == (0, 0)
        assert dev["vel_ratio"][3] == 0.125 and dev["acc_ratio"][3] == 0.0


def test_rows_with_a_nan_coordinate_are_counted_enter_no_extremum_and_are_never_eligible(engine, oracle, robots_):
    model, r, ro = robots_("wam")
    N, J = 12, 4
    Md, S = scoring.checked_states(N, J), model.nr_body_spheres()
    lim = _limits(7, mr.WAM_LIMITS)
    traj = mr.case_traj("wam", N, 5)
    clean = engine.motion_score_traj(r, lim, sr.DELTA_T, J, traj)
    bad = traj.copy()
    bad[3] = np.nan
    bad[1, 5, 2] = np.inf              # one joint of one support state
    bad[4, 7, 7 + 6] = np.nan          # one velocity of one support state
    dev = engine.motion_score_traj(r, lim, sr.DELTA_T, J, bad)
    exp = mr.oracle_motion_score(oracle, model, ro, mr.WAM_LIMITS, sr.DELTA_T, J, bad)
    assert np.array_equal(dev["invalid"], exp["invalid"]), (dev["invalid"], exp["invalid"])
    assert dev["invalid"][3] == 2 * Md * 7 + 2 * N * 7 + Md * S
    assert np.isposinf(dev["pos_margin"][3]) and dev["vel_ratio"][3] == 0 and dev["acc_ratio"][3] == 0
    assert dev["point_speed"][3] == 0 and dev["time_scale"][3] == 0 and (dev["worst"][3] == -1).all()
    # per coordinate: joint 2 of support state 5 spoils joint 2 in the 2 J + 1 states around it (their margins, the 2 J
    # interpolated velocities, the 4 acceleration ends of the two intervals) and the speeds of the 11 spheres behind
    # joint 2 there; the velocity of joint 6 at support state 7 the 2 J margins, 2 J + 1 velocities, 4 ends and the
    # speeds of the 6 spheres on the last link
    assert dev["invalid"][1] == (2 * J + 1) + 2 * J + 4 + (2 * J + 1) * 11
    assert dev["invalid"][4] == 2 * J + (2 * J + 1) + 4 + (2 * J + 1) * 6
    with np.errstate(invalid="ignore", over="ignore"):
        truth = mr.truth_motion_score(oracle, model, ro, mr.WAM_LIMITS, sr.DELTA_T, J, bad)
    for b in (1, 4):
        for k in mr.VALUES:
            e_gpu, e_cpu = mr.err(dev[k][b], truth[k][b]), mr.err(exp[k][b], truth[k][b])
            assert np.isfinite(dev[k][b]) and e_gpu <= min(mr.K * max(e_cpu, mr.FLOOR), mr.CAP), (b, k, e_gpu, e_cpu)
    _same_bits(dev, clean, rows=([0, 2], [0, 2]), what="ordinary rows beside rows with non-finite coordinates")
    fe = np.array([5.0, 1.0, 4.0, 0.5, 2.0])
    best, n = scoring.feasible_rule(fe, None, np.ones(5), None, pos_margin=dev["pos_margin"], time_scale=dev["time_scale"],
                                    motion_invalid=dev["invalid"], required_pos_margin=-np.inf, max_time_scale=np.inf)
    assert (best, n) == (2, 2)


def test_without_limits_nothing_is_limited(engine, robots_):
    model, r, _ = robots_("wam")
    traj = mr.case_traj("wam", 12, 3)
    for lim in (None, E.MotionLimits(7), E.MotionLimits(7, pos_down=-np.inf, pos_up=np.inf, vel=np.inf, acc=np.inf)):
        dev = engine.motion_score_traj(r, lim, sr.DELTA_T, 4, traj)
        assert np.isposinf(dev["pos_margin"]).all() and (dev["vel_ratio"] == 0).all() and (dev["acc_ratio"] == 0).all()
        assert np.isfinite(dev["point_speed"]).all() and (dev["point_speed"] > 0).all() and (dev["time_scale"] == 0).all()
        assert (dev["worst"][:, :3] == -1).all() and (dev["worst"][:, 3] >= 0).all() and (dev["invalid"] == 0).all()
    with_limits = engine.motion_score_traj(r, _limits(7, mr.WAM_LIMITS), sr.DELTA_T, 4, traj)
    assert np.array_equal(with_limits["point_speed"].view(np.int64), dev["point_speed"].view(np.int64))


def test_limit_arrays_are_checked_with_a_live_robot(engine, robots_):
    model, r, _ = robots_("wam")
    lib = engine.lib
    t = np.zeros((2, 3, 14))
    out = np.full(2, 7.0)
    seven = [E.dptr(out)] + [None] * 6
    good = np.ones(7)

    def call(**kw):
        a = {k: E.dptr(np.ascontiguousarray(v, dtype=np.float64)) for k, v in kw.items()}
        lim = _capi.MotionLimitsC(a.get("pos_down"), a.get("pos_up"), a.get("vel"), a.get("acc"), np.inf)
        return lib.gpmp2mi_motion_score_traj(r.ptr, C.byref(lim), 0.1, 1, 2, 2, E.dptr(t), *seven)
    nan_at = lambda i: np.where(np.arange(7) == i, np.nan, 1.0)
    assert call(pos_down=-good, pos_up=nan_at(6)) == 1 and call(pos_down=nan_at(0), pos_up=2 * good) == 1
    assert call(pos_down=np.where(np.arange(7) == 3, 1.5, -1.0), pos_up=good) == 1          # down > up
    assert call(vel=nan_at(2)) == 1 and call(vel=np.where(np.arange(7) == 2, 0.0, 1.0)) == 1 and call(vel=-good) == 1
    assert call(acc=nan_at(5)) == 1 and call(acc=np.where(np.arange(7) == 5, -1.0, 1.0)) == 1
    assert (out == 7.0).all()                                                                  # a refused call writes nothing
    assert call(pos_down=good, pos_up=good, vel=good, acc=good) == 0 and (out != 7.0).all()   # down == up is a limit
    out[:] = 7.0
    lim = _capi.MotionLimitsC(None, None, None, None, np.inf)
    assert lib.gpmp2mi_motion_score_traj(r.ptr, C.byref(lim), 0.1, 1, 0, 2, E.dptr(t), *seven) == 0 and (out == 7.0).all()   # B = 0
    assert lib.gpmp2mi_motion_score_traj(r.ptr, C.byref(lim), 0.1, 1, 2, 2, E.dptr(t), *([None] * 7)) == 0               # all NULL


def _args(p):
    return p.start_conf, p.start_vel, p.end_conf, p.end_vel


@pytest.fixture(scope="module")
def wam16(engine, oracle):
    """the 16-row WAM input of the issue solved on the device, with the reference's scores of that result"""
    p, J = ref.motivation_inputs()[0]
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pl = engine.plan(r, s, p.setting, p.B)
    pl.set_problem(*_args(p), p.init)
    pl.optimize()
    res = pl.result()
    ro = oracle.robot(p.model)
    dt = ref.delta_t(p.setting)
    return dict(p=p, J=J, r=r, s=s, pl=pl, res=res, dt=dt, ro=ro, lim=_limits(7, mr.WAM_LIMITS),
                pairs=engine.generate_self_pairs(r, 2, np.zeros((1, 7))),
                motion=mr.oracle_motion_score(oracle, p.model, ro, mr.WAM_LIMITS, dt, J, res["traj"]),
                truth=mr.truth_motion_score(oracle, p.model, ro, mr.WAM_LIMITS, dt, J, res["traj"]))


def test_a_row_scores_the_same_bits_alone_in_a_batch_and_through_the_plan(engine, wam16):
    w = wam16
    pl, r, lim, dt, J, traj = w["pl"], w["r"], w["lim"], w["dt"], w["J"], w["res"]["traj"]
    through_plan = pl.motion_score(lim, J)
    _check_against_reference(through_plan, w["motion"], "wam16 through the plan", w["truth"])
    batch = engine.motion_score_traj(r, lim, dt, J, traj)
    _same_bits(through_plan, batch, what="Plan.motion_score vs Engine.motion_score_traj on the fetched result")
    _same_bits(through_plan, pl.motion_score(lim, J), what="Plan.motion_score twice in a row")
    _same_bits(engine.motion_score_traj(r, lim, dt, J, traj[11]), batch, rows=(0, 11), what="alone vs row 11 of 16")
    big = np.repeat(traj, 16, axis=0)                    # 256 rows
    _same_bits(engine.motion_score_traj(r, lim, dt, J, big), batch, rows=(11 * 16 + 5, 11), what="in a batch of 256")
    part = pl.motion_score(lim, J, out={"time_scale": np.zeros(16)})     # only the outputs asked for are written
    assert np.array_equal(part["time_scale"].view(np.int64), through_plan["time_scale"].view(np.int64))
    pl.motion_score(lim, 9)                              # another inter_step grows the workspace
    _same_bits(through_plan, pl.motion_score(lim, J), what="after the workspace grew")
    assert (through_plan["time_scale"] > 1.0).all()      # no row of this input is executable as planned


def test_select_feasible_is_the_extended_rule_on_the_devices_own_scores(engine, wam16):
    w = wam16
    pl, pairs, lim, J, res = w["pl"], w["pairs"], w["lim"], w["J"], w["res"]
    ob, se, mo = pl.score(J), pl.self_score(pairs, J), pl.motion_score(lim, J)
    fe, st = res["final_error"], res["status"]
    seen = set()
    for req, rir, use_pairs, req_self, rpm, mts in (
            (0.0, False, False, 0.0, 0.0, np.inf), (0.0, True, True, 0.0, 0.0, np.inf), (0.0, False, False, 0.0, -np.inf, 2.4),
            (-np.inf, False, True, -np.inf, -0.1, 2.45), (0.0, False, False, 0.0, 0.1, 3.0), (0.0, False, True, 0.0, 0.0, 1.0),
            (0.02, True, False, 0.0, -np.inf, float(np.median(mo["time_scale"])))):
        want = scoring.feasible_rule(fe, st, ob["min_clearance"], ob["out_of_range"], req, rir,
                                     se["min_self_clearance"] if use_pairs else None, se["invalid"] if use_pairs else None,
                                     req_self, mo["pos_margin"], mo["time_scale"], mo["invalid"], rpm, mts)
        got = pl.select_feasible(J, lim, rpm, mts, req, rir, pairs if use_pairs else None, req_self)
        print((req, rir, use_pairs, req_self, rpm, mts), "->", got["best"], got["n_eligible"], got["time_scale_best"])
        assert (got["best"], got["n_eligible"]) == want, (req, rir, use_pairs, req_self, rpm, mts, want)
        seen.add(want)
        if want[0] >= 0:
            assert got["time_scale_best"] == mo["time_scale"][want[0]]
            assert np.array_equal(got["traj_best"].view(np.int64), res["traj"][want[0]].view(np.int64))
            plain = pl.select(J, -np.inf, False)
            if plain["best"] == want[0]:
                assert np.array_equal(got["dense_best"].view(np.int64), plain["dense_best"].view(np.int64))
        else:
            assert got["time_scale_best"] is None and got["traj_best"] is None and got["dense_best"] is None
    assert len(seen) >= 3 and (-1, 0) in seen          # the thresholds told rows apart, and one refused them all


def test_without_limits_select_feasible_is_select_and_select_checked(engine, wam16):
    w = wam16
    pl, pairs, J = w["pl"], w["pairs"], w["J"]
    for req, rir in ((0.0, False), (0.0, True), (0.02, False), (10.0, False)):
        a, b = pl.select(J, req, rir), pl.select_feasible(J, None, -np.inf, np.inf, req, rir)
        c, d = pl.select_checked(J, pairs, req, rir, 0.0), pl.select_feasible(J, None, -np.inf, np.inf, req, rir, pairs, 0.0)
        for x, y in ((a, b), (c, d)):
            assert (x["best"], x["n_eligible"]) == (y["best"], y["n_eligible"])
            for k in ("traj_best", "dense_best"):
                assert (x[k] is None and y[k] is None) or np.array_equal(x[k], y[k]), k


def test_the_existing_calls_are_left_alone(engine, wam16):
    """plan.score / select before and after the new calls, and update(1) with and without them in front: array_equal"""
    w = wam16
    p, r, s, pairs, lim, J = w["p"], w["r"], w["s"], w["pairs"], w["lim"], w["J"]
    plans = []
    for with_motion in (False, True):
        pl = engine.plan(r, s, p.setting, p.B)
        pl.set_problem(*_args(p), p.init)
        pl.optimize()
        before, sel_before = pl.score(J), pl.select(J, 0.0, True)
        if with_motion:
            pl.motion_score(lim, J)
            pl.select_feasible(J, lim, 0.0, 3.0, 0.0, True, pairs, 0.0)
            pl.select_feasible(J, lim, 0.0, 3.0)
            after, sel_after = pl.score(J), pl.select(J, 0.0, True)
            for k in scoring.SCORE_NAMES:
                assert np.array_equal(before[k], after[k]), k
            assert (sel_before["best"], sel_before["n_eligible"]) == (sel_after["best"], sel_after["n_eligible"])
            assert np.array_equal(sel_before["dense_best"], sel_after["dense_best"])
        pl.update(1)
        plans.append((pl, pl.result()))
    for k in ("traj", "final_error", "iters", "status"):
        assert np.array_equal(plans[0][1][k], plans[1][1][k]), k
    for pl, _ in plans:
        pl.close()


def test_plan_states_and_refusals(engine, wam16, robots_):
    w = wam16
    p, r, s, pairs, lim, J = w["p"], w["r"], w["s"], w["pairs"], w["lim"], w["J"]
    pl = engine.plan(r, s, p.setting, p.B)
    for call in (lambda: pl.motion_score(lim, J), lambda: pl.select_feasible(J, lim)):     # nothing to score yet
        with pytest.raises(E.Gpmp2miError) as ei:
            call()
        assert ei.value.code == 1 and "not been optimized" in str(ei.value)
    pl.set_problem(*_args(p), p.init)
    pl.optimize()
    _, r3, _ = robots_("arm3s")
    other = engine.self_pairs(r3, [[0, 5, 0, 1]])
    with pytest.raises(E.Gpmp2miError) as ei:
        pl.select_feasible(J, lim, pairs=other)
    assert ei.value.code == 1 and "another robot" in str(ei.value)
    lib = engine.lib
    bad = _capi.MotionLimitsC(None, None, E.dptr(np.zeros(7)), None, np.inf)
    assert lib.gpmp2mi_plan_motion_score(pl.h.ptr, C.byref(bad), J, *([None] * 7)) == 1
    assert lib.gpmp2mi_plan_motion_score(pl.h.ptr, C.byref(lim.c), -1, *([None] * 7)) == 1
    assert lib.gpmp2mi_plan_motion_score(pl.h.ptr, C.byref(lim.c), J, *([None] * 7)) == 0          # every output may be NULL
    assert lib.gpmp2mi_plan_select_feasible(pl.h.ptr, J, 0.0, 0, None, 0.0, C.byref(lim.c), 0.0, 3.0, None, None, None, None, None) == 0
    assert pl.motion_score(lim, J)["invalid"].sum() == 0                                          # the plan is as usable as before
    pl.optimize_queue(*_args(p), p.init)          # a queue run leaves no problem behind
    with pytest.raises(E.Gpmp2miError) as ei:
        pl.motion_score(lim, J)
    assert ei.value.code == 1
    pl.close()


_DEV = r"""
import numpy as np
import torch                      # torch's HIP runtime first, as bench.py does
torch.cuda.init()
import sys
sys.path.insert(0, "tests")
import motion_reference as mr
from gpmp2_amd import engine as E, problems
eng = E.Engine()
p = problems.wam_restarts(B=5, total_step=12, obs_check_inter=3, opt="GN", sdf="40")
r, s = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
pl = eng.plan(r, s, p.setting, p.B)
pl.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
pl.optimize()
B, N, D, J = p.B, p.setting.total_step, 7, 4
Md = N * (J + 1) + 1
lim = E.MotionLimits(7, **mr.WAM_LIMITS)
pairs = eng.generate_self_pairs(r, 2, np.zeros((1, 7)))
host = pl.motion_score(lim, J)
mts = float(np.sort(host["time_scale"])[2])
sel = pl.select_feasible(J, lim, -np.inf, mts, 0.0, False, pairs, -np.inf)
assert sel["best"] >= 0
dev = torch.device("cuda:0")
nan = float("nan")
f = lambda *shape: torch.full(shape, nan, dtype=torch.float64, device=dev)
i = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device=dev)
o = dict(pos_margin=f(B), vel_ratio=f(B), acc_ratio=f(B), point_speed=f(B), time_scale=f(B), worst=i(B, 4, 2), invalid=i(B))
best, n, ts, tb, db = i(1), i(1), f(1), f(N + 1, 2 * D), f(Md, 2 * D)
torch.cuda.synchronize()
st = torch.cuda.Stream(device=dev)
pl.motion_score_dev(lim, J, stream=st.cuda_stream, **o)
pl.select_feasible_dev(J, lim, -np.inf, mts, 0.0, False, pairs, -np.inf, best, n, ts, tb, db, stream=st.cuda_stream)
with torch.cuda.stream(st):
    got = {k: t.cpu().numpy() for k, t in o.items()}
    pick = [t.cpu().numpy() for t in (best, n, ts, tb, db)]
bits = lambda a: np.ascontiguousarray(a).view(np.int64) if a.dtype == np.float64 else a
for k in host:
    assert np.array_equal(bits(got[k]), bits(host[k])), "motion_score_dev != motion_score: " + k
assert (int(pick[0][0]), int(pick[1][0])) == (sel["best"], sel["n_eligible"])
assert pick[2][0] == sel["time_scale_best"]
assert np.array_equal(bits(pick[3]), bits(sel["traj_best"])) and np.array_equal(bits(pick[4]), bits(sel["dense_best"]))
# any output may be None; a threshold no row meets leaves the outputs about the chosen row alone
pl.motion_score_dev(lim, J, time_scale=o["time_scale"], stream=st.cuda_stream)
pl.select_feasible_dev(J, lim, 0.0, 1e-3, time_scale_best=ts, traj_best=tb, n_eligible=n, stream=st.cuda_stream)
st.synchronize()
assert int(n.cpu()[0]) == 0 and float(ts.cpu()[0]) == sel["time_scale_best"]
assert np.array_equal(bits(tb.cpu().numpy()), bits(sel["traj_best"]))
# the trajectory form with device pointers
traj = torch.from_numpy(pl.result()["traj"]).to(dev)
out = f(B)
lib = eng.lib
rc = lib.gpmp2mi_motion_score_traj_dev(r.ptr, lim.ref(7), p.setting.total_time / N, J, B, N, traj.data_ptr(), None, None, None,
                                       None, out.data_ptr(), None, None, st.cuda_stream)
assert rc == 0
st.synchronize()
assert np.array_equal(bits(out.cpu().numpy()), bits(host["time_scale"]))
pl.close()
print("MOTION DEV OK")
"""


def test_dev_forms_equal_the_host_calls_bit_for_bit():
    """motion_score_dev / select_feasible_dev into torch tensors on a torch stream; in a fresh process that starts torch's
    HIP runtime before the library, as bench.py does"""
    assert importlib.util.find_spec("torch") is not None    # not imported here: this process keeps the library's runtime
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + [x for x in [os.environ.get("PYTHONPATH")] if x]))
    r = subprocess.run([sys.executable, "-c", _DEV], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0 and "MOTION DEV OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
