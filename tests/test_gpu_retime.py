"""Re-timing on the device (include/gpmp2mi.h "re-timing") through every entry point.

 - gpmp2mi_retime_path against gpmp2_amd/csrc/retime_rule.h built by the host compiler (tests/retime_shim.py): every
   output bit for bit, on the adversarial inputs of tests/test_retime_cpu.py (a pause, rest at both ends, more pairs than
   lanes, more states than a tile, no limit on a joint, forced rates, rows that are not OK).
 - gpmp2mi_retime_traj / gpmp2mi_plan_retime against the numpy rule (tests/retime_reference.py) fed from the same traj,
   with the CPU oracle's interpolation and Jacobians behind ps: sdot, stamps and duration within
   max(1e-12 relative, 10 x the numpy rule's own change under a 2-ulp perturbation of traj), the device of
   tests/parity_bound.py with the same factor 10.  No more than one row in twenty may need the second clause; the test
   prints and asserts the count (measured table: scripts/retime_error.py -> profiles/retime_error.txt).
 - the properties of the rule recomputed in numpy from the device's own outputs, batch independence, the selection, the
   refusals, and that the existing calls are left alone."""
import ctypes as C

import numpy as np
import pytest

import motion_reference as mr
import retime_reference as rr
import retime_shim
import self_reference as sr
from gpmp2_amd import _capi, problems, scoring
from gpmp2_amd import engine as E

pytestmark = pytest.mark.gpu
PATH_CASES = rr.path_cases()
MAX_RATE = 4.0
PROFILE = ("sdot", "u", "stamps", "duration", "status", "achieved")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same_bits(a, b, names, rows=None, what=""):
    for k in names:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows[0]], b[k][rows[1]])
        assert np.array_equal(_bits(x), _bits(y)), (what, k, x, y)


def _limits(D, lim):
    return E.MotionLimits(D, **{k: v for k, v in lim.items() if v is not None and k in ("vel", "acc", "point_speed")})


@pytest.fixture(scope="module")
def robots_(engine, oracle):
    made = {}

    def get(name):
        if name not in made:
            model = mr.models()[name]()
            made[name] = (model, engine.robot(model), oracle.robot(model))
        return made[name]
    return get


# ---------------------------------------------------------------------------------------------------------- the bare rule
@pytest.mark.parametrize("name", [n for n, _ in PATH_CASES])
def test_retime_path_gives_the_bits_of_the_host_rule(engine, name):
    c = dict(PATH_CASES)[name]
    D = c["traj"].shape[1] // 2
    qd, qL, qR, h = rr.path_from_traj(c["traj"], c["dt"], c["J"])
    cap = rr.rate_caps(qd, c["vel"])
    rest = not c["traj"][0, D:].any() and not c["traj"][-1, D:].any()
    ends = [dict(), dict(max_rate=1.0), dict(rate_end=0.125), dict(rate_start=0.25, rate_end=0.25),
            dict(rate_start=MAX_RATE * 1.01)]
    if rest:
        ends.append(dict(rate_start=0.0, rate_end=0.0))
    seen = set()
    for kw in ends:
        kw = dict(dict(max_rate=MAX_RATE), **kw)
        host = retime_shim.retime_path(qd, qL, qR, cap, c["acc"], h, **kw)
        dev = engine.retime_path(qd, qL, qR, cap, c["acc"], h, **kw)
        one = {k: dev[k][0] for k in PROFILE}
        host["status"] = np.int32(host["status"])
        _same_bits(one, host, PROFILE, what=(name, kw))
        seen.add(int(one["status"]))
    assert seen >= {rr.OK, rr.BOUNDARY}


def test_retime_path_rows_do_not_see_each_other(engine):
    """five rows of one shape, one of them with a NaN and one that cannot be passed: every row has the bits of the host
    rule and of the same row alone"""
    rng = np.random.default_rng(5)
    N, D, J, dt = 6, 7, 2, 0.5
    vel, acc = np.full(D, 1.0), np.full(D, 2.0)
    rows = [rr.path_from_traj(rr.random_traj(rng, N, D, dt, rest=True, pause=b == 1), dt, J) for b in range(5)]
    h = rows[0][3]
    qd, qL, qR = (np.ascontiguousarray([r[i] for r in rows]) for i in range(3))
    cap = np.ascontiguousarray([rr.rate_caps(r[0], vel) for r in rows])
    qd[3, 4, 2] = np.nan
    qL[2, -1] = 400.0                       # row 2 ends at rest with an acceleration that the forced end rate breaks
    dev = engine.retime_path(qd, qL, qR, cap, acc, h, max_rate=MAX_RATE, rate_end=0.125)
    for b in range(5):
        host = retime_shim.retime_path(qd[b], qL[b], qR[b], cap[b], acc, h, max_rate=MAX_RATE, rate_end=0.125)
        host["status"] = np.int32(host["status"])
        _same_bits({k: dev[k][b] for k in PROFILE}, host, PROFILE, what=b)
        alone = engine.retime_path(qd[b], qL[b], qR[b], cap[b], acc, h, max_rate=MAX_RATE, rate_end=0.125)
        _same_bits(alone, dev, PROFILE, rows=(0, b), what=("alone", b))
    assert dev["status"][3] == rr.INVALID and dev["status"][2] == rr.EMPTY and (dev["status"][[0, 1, 4]] == rr.OK).all()
    assert np.isinf(dev["duration"][[2, 3]]).all() and np.isnan(dev["sdot"][[2, 3]]).all()


# ------------------------------------------------------------------------------------------ trajectories against numpy
TRAJ_CASES = [("arm3", (5, 2), 3), ("point1", (2, 0), 3), ("wam", (8, 4), 5), ("wam", (20, 4), 2), ("wam", (6, 1), 5),
              ("wam", (5, 0), 5)]


def _reference(oracle, model, ro, lim, dt, J, traj, **kw):
    ps = rr.sphere_speeds(oracle, model, ro, traj, dt, J)
    _, _, vel, acc, point_speed = mr.expand(lim, model.dof())
    return [rr.retime_traj(traj[b], dt, J, vel, acc, point_speed, ps[b], **kw) for b in range(traj.shape[0])], ps


@pytest.fixture(scope="module")
def clause_count():
    count = dict(rows=0, second=0)
    yield count
    print("rows compared", count["rows"], "of which the sensitivity clause was needed for", count["second"])


@pytest.mark.parametrize("case", TRAJ_CASES, ids=[mr.case_id(c) for c in TRAJ_CASES])
def test_retime_traj_matches_the_numpy_rule(engine, oracle, robots_, clause_count, case):
    name, (N, J), B = case
    model, r, ro = robots_(name)
    D = model.dof()
    lim, dt = mr.case_limits(name), mr.case_dt(name)
    traj = mr.case_traj(name, N, B)
    kw = dict(max_rate=2.0)
    dev = engine.retime_traj(r, _limits(D, lim), dt, J, traj, **kw)
    ref, ps = _reference(oracle, model, ro, lim, dt, J, traj, **kw)
    moved, _ = _reference(oracle, model, ro, lim, dt, J, rr.ulp_perturbed(traj, np.random.default_rng(3)), **kw)
    second = 0
    for b in range(B):
        assert dev["status"][b] == ref[b]["status"] == rr.OK, (b, dev["status"][b], ref[b]["status"])
        needs = False
        for k in ("sdot", "stamps", "duration"):
            x, y, z = np.asarray(dev[k][b]), np.asarray(ref[b][k]), np.asarray(moved[b][k])
            e, rel, sens = np.abs(x - y), 1e-12 * np.abs(y), 10.0 * np.abs(z - y)
            print(f"{mr.case_id(case)} row {b} {k}: err {e.max():.2e}, err / 1e-12 rel {np.max(e / np.maximum(rel, 1e-300)):.2e}")
            assert (e <= np.maximum(rel, sens)).all(), (b, k, e.max(), rel.max(), sens.max())
            needs = needs or bool((e > rel).any())
        second += needs
        # the rule's properties, recomputed in numpy from the device's own profile
        qd, qL, qR, h = rr.path_from_traj(traj[b], dt, J)
        _, _, vel, acc, point_speed = mr.expand(lim, D)
        cap = rr.rate_caps(qd, vel, ps[b], point_speed)
        ach = rr.achieved(qd, qL, qR, cap, acc, h, dev["sdot"][b] ** 2, dev["u"][b], vel, ps[b], point_speed)
        assert ach[0] <= 1 + 1e-9 and ach[1] <= 1 + 1e-9 and ach[3] <= 1 + 1e-9, ach
        np.testing.assert_allclose(dev["achieved"][b], ach, rtol=1e-12, atol=0)
        assert dev["duration"][b] == dev["stamps"][b, -1] and dev["stamps"][b, 0] == 0 and (np.diff(dev["stamps"][b]) > 0).all()
        assert (dev["sdot"][b] <= 2.0).all()
        U = oracle.interpolate_traj(D, False, None, dt, J, traj[b:b + 1])[0]
        np.testing.assert_allclose(dev["dense_retimed"][b][:, :D], U[:, :D], rtol=0, atol=1e-13)
        np.testing.assert_allclose(dev["dense_retimed"][b][:, D:], U[:, D:] * dev["sdot"][b][:, None], rtol=0, atol=1e-12)
    clause_count["rows"] += B
    clause_count["second"] += second
    # a row alone, and at the end of another batch: the same bits
    b = B // 2
    names = PROFILE + ("dense_retimed",)
    _same_bits(engine.retime_traj(r, _limits(D, lim), dt, J, traj[b], **kw), dev, names, rows=(0, b), what="alone")
    shuffled = np.concatenate([traj[b + 1:], traj[:b + 1], traj[b:b + 1]])
    _same_bits(engine.retime_traj(r, _limits(D, lim), dt, J, shuffled, **kw), dev, names, rows=(B, b), what="shuffled")


def test_no_more_than_one_row_in_twenty_needed_the_sensitivity_clause(clause_count):
    """runs behind the cases above (file order)"""
    assert clause_count["rows"] == sum(c[2] for c in TRAJ_CASES)
    assert 20 * clause_count["second"] <= clause_count["rows"], clause_count


def test_uniform_stretch_forced_rates_and_max_rate(engine, oracle, robots_):
    model, r, ro = robots_("wam")
    N, J, B, dt = 8, 4, 5, sr.DELTA_T
    lim = mr.WAM_LIMITS
    traj = mr.case_traj("wam", N, B)
    traj[:, 0, 7:] = 0.0
    traj[:, -1, 7:] = 0.0
    L = _limits(7, lim)
    total = N * dt
    scale = engine.motion_score_traj(r, L, dt, J, traj)["time_scale"]
    free = engine.retime_traj(r, L, dt, J, traj, max_rate=MAX_RATE)
    assert (free["status"] == rr.OK).all()
    assert (free["duration"] <= np.maximum(scale, 1.0 / MAX_RATE) * total * (1 + 1e-12)).all(), (free["duration"], scale * total)
    print("re-timed / uniform", free["duration"] / (np.maximum(scale, 1.0 / MAX_RATE) * total))
    one = engine.retime_traj(r, L, dt, J, traj, max_rate=1.0)
    assert (one["status"] == rr.OK).all() and (one["sdot"] <= 1.0).all() and (one["duration"] >= total * (1 - 1e-12)).all()
    rest = engine.retime_traj(r, L, dt, J, traj, max_rate=MAX_RATE, rate_start=0.0, rate_end=0.0)
    assert (rest["status"] == rr.OK).all() and (rest["sdot"][:, [0, -1]] == 0).all()
    assert (rest["duration"] >= free["duration"]).all() and np.isfinite(rest["duration"]).all()
    over = engine.retime_traj(r, L, dt, J, traj, max_rate=MAX_RATE, rate_start=MAX_RATE * 1.01)
    assert (over["status"] == rr.BOUNDARY).all() and np.isinf(over["duration"]).all() and np.isnan(over["stamps"]).all()
    assert np.isnan(over["dense_retimed"][:, :, 7:]).all() and np.isfinite(over["dense_retimed"][:, :, :7]).all()
    none = engine.retime_traj(r, None, dt, J, traj, max_rate=2.0)          # no limit: the cap alone
    assert (none["sdot"] == 2.0).all() and np.allclose(none["duration"], total / 2.0, rtol=1e-13)


def test_a_nan_row_is_invalid_and_leaves_the_others_alone(engine, robots_):
    model, r, _ = robots_("wam")
    N, J, dt = 6, 1, sr.DELTA_T
    L = _limits(7, mr.WAM_LIMITS)
    traj = mr.case_traj("wam", N, 5)
    clean = engine.retime_traj(r, L, dt, J, traj, max_rate=2.0)
    bad = traj.copy()
    bad[1, 3, 2] = np.nan
    bad[3, 5, 7 + 4] = np.inf
    dev = engine.retime_traj(r, L, dt, J, bad, max_rate=2.0)
    assert list(dev["status"]) == [0, rr.INVALID, 0, rr.INVALID, 0]
    assert np.isinf(dev["duration"][[1, 3]]).all() and np.isnan(dev["sdot"][[1, 3]]).all()
    assert np.isnan(dev["achieved"][[1, 3]]).all() and np.isnan(dev["u"][[1, 3]]).all()
    _same_bits(dev, clean, PROFILE + ("dense_retimed",), rows=([0, 2, 4], [0, 2, 4]), what="rows beside a NaN row")


def test_refusals_with_a_live_robot(engine, robots_):
    model, r, _ = robots_("wam")
    lib = engine.lib
    t = np.zeros((2, 3, 14))
    out = np.full((2, 3), 7.0)
    seven = [E.dptr(out)] + [None] * 6
    bad = _capi.MotionLimitsC(None, None, None, E.dptr(np.where(np.arange(7) == 5, -1.0, 1.0)), np.inf)
    assert lib.gpmp2mi_retime_traj(r.ptr, C.byref(bad), 0.1, 0, 2, 2, E.dptr(t), 1.0, -1.0, -1.0, *seven) == 1
    ok = _capi.MotionLimitsC(None, None, None, None, np.inf)
    assert lib.gpmp2mi_retime_traj(r.ptr, C.byref(ok), 0.1, 0, 0, 2, E.dptr(t), 1.0, -1.0, -1.0, *seven) == 0      # B = 0
    _, mobile, _ = robots_("config5")
    t5 = np.zeros((2, 3, 10))
    assert lib.gpmp2mi_retime_traj(mobile.ptr, C.byref(ok), 0.1, 0, 2, 2, E.dptr(t5), 1.0, -1.0, -1.0, *seven) == 4
    assert b"Pose2" in lib.gpmp2mi_last_error() and b"tangent-space" in lib.gpmp2mi_last_error()
    assert (out == 7.0).all()                                                                 # a refused call writes nothing
    with pytest.raises(E.Gpmp2miError) as ei:
        engine.retime_traj(mobile, None, 0.1, 0, t5)
    assert ei.value.code == 4
    assert lib.gpmp2mi_retime_traj(r.ptr, C.byref(ok), 0.1, 0, 2, 2, E.dptr(t), 1.0, -1.0, -1.0, *([None] * 7)) == 0   # all NULL


# ------------------------------------------------------------------------------------------------------------ the plan
def _args(p):
    return p.start_conf, p.start_vel, p.end_conf, p.end_vel


@pytest.fixture(scope="module")
def wam8(engine):
    """eight restarts of a small WAM problem solved on the device"""
    p = problems.wam_restarts(B=8, total_step=12, obs_check_inter=3, opt="GN", sdf="40")
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pl = engine.plan(r, s, p.setting, p.B)
    pl.set_problem(*_args(p), p.init)
    pl.optimize()
    return dict(p=p, J=4, r=r, s=s, pl=pl, res=pl.result(), dt=p.setting.total_time / p.setting.total_step,
                lim=_limits(7, mr.WAM_LIMITS), pairs=engine.generate_self_pairs(r, 2, np.zeros((1, 7))))


def test_plan_form_has_the_bits_of_the_trajectory_form(engine, wam8):
    w = wam8
    pl, r, lim, dt, J, traj = w["pl"], w["r"], w["lim"], w["dt"], w["J"], w["res"]["traj"]
    names = PROFILE + ("dense_retimed",)
    through_plan = pl.retime(lim, J, max_rate=2.0)
    assert (through_plan["status"] == rr.OK).all()
    batch = engine.retime_traj(r, lim, dt, J, traj, max_rate=2.0)
    _same_bits(through_plan, batch, names, what="Plan.retime vs Engine.retime_traj on the fetched result")
    _same_bits(through_plan, pl.retime(lim, J, max_rate=2.0), names, what="Plan.retime twice in a row")
    _same_bits(engine.retime_traj(r, lim, dt, J, traj[5], max_rate=2.0), batch, names, rows=(0, 5), what="alone vs row 5 of 8")
    part = pl.retime(lim, J, max_rate=2.0, out={"duration": np.zeros(8)})
    assert np.array_equal(_bits(part["duration"]), _bits(through_plan["duration"]))
    pl.retime(lim, 7, max_rate=2.0)                      # another inter_step grows the workspace
    _same_bits(through_plan, pl.retime(lim, J, max_rate=2.0), names, what="after the workspace grew")
    scale = pl.motion_score(lim, J)["time_scale"]
    total = w["p"].setting.total_time
    print("uniform", scale * total, "re-timed", through_plan["duration"])
    assert (through_plan["duration"] <= np.maximum(scale, 0.5) * total * (1 + 1e-12)).all()


def test_select_retimed_is_the_rule_on_the_devices_own_scores(engine, wam8):
    w = wam8
    pl, pairs, lim, J, res = w["pl"], w["pairs"], w["lim"], w["J"], w["res"]
    ob, se, mo = pl.score(J), pl.self_score(pairs, J), pl.motion_score(lim, J)
    rt = pl.retime(lim, J, max_rate=2.0)
    fe, st = res["final_error"], res["status"]
    med = float(np.median(rt["duration"]))
    seen = set()
    for req, rir, use_pairs, req_self, rpm, md in (
            (0.0, False, False, 0.0, -np.inf, np.inf), (0.0, True, True, 0.0, -np.inf, np.inf), (0.0, False, False, 0.0, -np.inf, med),
            (-np.inf, False, True, -np.inf, -0.1, med), (0.0, False, False, 0.0, 0.0, np.inf),
            (0.0, False, False, 0.0, -np.inf, float(rt["duration"].min()) * 0.99), (-np.inf, False, False, 0.0, -np.inf, float(rt["duration"].min()))):
        want = scoring.retimed_rule(fe, st, ob["min_clearance"], ob["out_of_range"], req, rir,
                                    se["min_self_clearance"] if use_pairs else None, se["invalid"] if use_pairs else None,
                                    req_self, mo["pos_margin"], mo["invalid"], rpm, rt["status"], rt["duration"], md)
        got = pl.select_retimed(J, lim, rpm, md, 2.0, None, None, req, rir, pairs if use_pairs else None, req_self)
        print((req, rir, use_pairs, req_self, rpm, md), "->", got["best"], got["n_eligible"], got["duration_best"])
        assert (got["best"], got["n_eligible"]) == want, (req, rir, use_pairs, req_self, rpm, md, want)
        seen.add(want)
        if want[0] >= 0:
            b = want[0]
            assert got["duration_best"] == rt["duration"][b]
            assert np.array_equal(_bits(got["stamps_best"]), _bits(rt["stamps"][b]))
            assert np.array_equal(_bits(got["traj_best"]), _bits(res["traj"][b]))
            assert np.array_equal(_bits(got["dense_best"]), _bits(rt["dense_retimed"][b]))
        else:
            assert got["duration_best"] is None and got["stamps_best"] is None and got["dense_best"] is None
        if md == np.inf:        # every row re-times OK: the rule of select_feasible without a bound on time_scale
            feas = pl.select_feasible(J, lim, rpm, np.inf, req, rir, pairs if use_pairs else None, req_self)
            assert (feas["best"], feas["n_eligible"]) == (got["best"], got["n_eligible"])
    assert len(seen) >= 3 and (-1, 0) in seen          # the thresholds told rows apart, and one refused them all
    # a forced start rate no row can take: nothing is eligible, whatever the duration bound
    none = pl.select_retimed(J, lim, -np.inf, np.inf, 2.0, 2.5, None, -np.inf)
    assert (none["best"], none["n_eligible"]) == (-1, 0)


def test_the_existing_calls_are_left_alone(engine, wam8):
    """plan.score / select_feasible before and after the new calls, and update(1) with and without them in front"""
    w = wam8
    p, r, s, pairs, lim, J = w["p"], w["r"], w["s"], w["pairs"], w["lim"], w["J"]
    plans = []
    for with_retime in (False, True):
        pl = engine.plan(r, s, p.setting, p.B)
        pl.set_problem(*_args(p), p.init)
        pl.optimize()
        before, sel_before = pl.score(J), pl.select_feasible(J, lim, -np.inf, 3.0)
        if with_retime:
            pl.retime(lim, J, max_rate=2.0)
            pl.select_retimed(J, lim, -np.inf, np.inf, 2.0, None, None, 0.0, True, pairs, 0.0)
            after, sel_after = pl.score(J), pl.select_feasible(J, lim, -np.inf, 3.0)
            for k in scoring.SCORE_NAMES:
                assert np.array_equal(before[k], after[k]), k
            assert (sel_before["best"], sel_before["n_eligible"]) == (sel_after["best"], sel_after["n_eligible"])
            if sel_before["best"] >= 0:
                assert np.array_equal(sel_before["dense_best"], sel_after["dense_best"])
        pl.update(1)
        plans.append((pl, pl.result()))
    for k in ("traj", "final_error", "iters", "status"):
        assert np.array_equal(plans[0][1][k], plans[1][1][k]), k
    for pl, _ in plans:
        pl.close()


def test_plan_states_and_refusals(engine, wam8):
    w = wam8
    p, r, s, lim, J = w["p"], w["r"], w["s"], w["lim"], w["J"]
    pl = engine.plan(r, s, p.setting, p.B)
    for call in (lambda: pl.retime(lim, J), lambda: pl.select_retimed(J, lim)):     # nothing to re-time yet
        with pytest.raises(E.Gpmp2miError) as ei:
            call()
        assert ei.value.code == 1 and "not been optimized" in str(ei.value)
    pl.set_problem(*_args(p), p.init)
    pl.optimize()
    lib = engine.lib
    bad = _capi.MotionLimitsC(None, None, E.dptr(np.zeros(7)), None, np.inf)
    assert lib.gpmp2mi_plan_retime(pl.h.ptr, C.byref(bad), J, 1.0, -1.0, -1.0, *([None] * 7)) == 1
    assert lib.gpmp2mi_plan_retime(pl.h.ptr, C.byref(lim.c), -1, 1.0, -1.0, -1.0, *([None] * 7)) == 1
    assert lib.gpmp2mi_plan_retime(pl.h.ptr, C.byref(lim.c), J, 1.0, -1.0, -1.0, *([None] * 7)) == 0      # every output may be NULL
    assert lib.gpmp2mi_plan_select_retimed(pl.h.ptr, J, 0.0, 0, None, 0.0, C.byref(lim.c), 0.0, 1.0, -1.0, -1.0, np.inf,
                                           *([None] * 6)) == 0
    assert (pl.retime(lim, J)["status"] == rr.OK).all()                                          # the plan is as usable as before
    pl.close()


# ------------------------------------------------------------------------------------------------------ the `_dev` forms
class _DevBuf:
    """a device buffer through the HIP runtime (ctypes), for the device-pointer entry points"""
    hip = None

    def __init__(self, a):
        if _DevBuf.hip is None:
            _DevBuf.hip = C.CDLL("libamdhip64.so")
        self.a = np.ascontiguousarray(a)
        self.ptr = C.c_void_p()
        assert _DevBuf.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(self.a.nbytes)) == 0
        assert _DevBuf.hip.hipMemcpy(self.ptr, self.a.ctypes.data_as(C.c_void_p), C.c_size_t(self.a.nbytes), 1) == 0

    def get(self):
        out = np.empty_like(self.a)
        assert _DevBuf.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.ptr, C.c_size_t(self.a.nbytes), 2) == 0
        return out

    def __del__(self):
        if self.ptr:
            _DevBuf.hip.hipFree(self.ptr)


def test_dev_forms_equal_the_host_calls_bit_for_bit(engine, wam8):
    """device buffers on the null stream; hipMemcpy back waits for it"""
    w = wam8
    pl, r, pairs, lim, J, dt = w["pl"], w["r"], w["pairs"], w["lim"], w["J"], w["dt"]
    B, N, D = 8, 12, 7
    Md = scoring.checked_states(N, J)
    host = pl.retime(lim, J, max_rate=2.0)
    shapes = dict(sdot=(B, Md), u=(B, Md), stamps=(B, Md), duration=(B,), status=(B,), achieved=(B, 4),
                  dense_retimed=(B, Md, 2 * D))

    def outs():
        return {k: _DevBuf(np.full(s, -7, dtype=np.int32) if k == "status" else np.full(s, np.nan)) for k, s in shapes.items()}
    o = outs()
    pl.retime_dev(lim, J, max_rate=2.0, **{k: v.ptr.value for k, v in o.items()})
    _same_bits({k: v.get() for k, v in o.items()}, host, shapes, what="Plan.retime_dev")
    o = outs()
    traj = _DevBuf(w["res"]["traj"])
    rc = engine.lib.gpmp2mi_retime_traj_dev(r.ptr, lim.ref(7), dt, J, B, N, traj.ptr, 2.0, -1.0, -1.0,
                                            *[o[k].ptr for k in shapes], None)
    assert rc == 0
    _same_bits({k: v.get() for k, v in o.items()}, host, shapes, what="gpmp2mi_retime_traj_dev")
    part = _DevBuf(np.full(B, np.nan))                   # any output may be NULL
    pl.retime_dev(lim, J, max_rate=2.0, duration=part.ptr.value)
    assert np.array_equal(_bits(part.get()), _bits(host["duration"]))
    md = float(np.sort(host["duration"])[3])
    sel = pl.select_retimed(J, lim, -np.inf, md, 2.0, None, None, 0.0, False, pairs, -np.inf)
    assert sel["best"] >= 0
    best, n = _DevBuf(np.full(1, -7, dtype=np.int32)), _DevBuf(np.full(1, -7, dtype=np.int32))
    dur, sb = _DevBuf(np.full(1, np.nan)), _DevBuf(np.full(Md, np.nan))
    tb, db = _DevBuf(np.full((N + 1, 2 * D), np.nan)), _DevBuf(np.full((Md, 2 * D), np.nan))
    pl.select_retimed_dev(J, lim, -np.inf, md, 2.0, None, None, 0.0, False, pairs, -np.inf, best.ptr.value, n.ptr.value,
                          dur.ptr.value, sb.ptr.value, tb.ptr.value, db.ptr.value)
    assert (int(best.get()[0]), int(n.get()[0])) == (sel["best"], sel["n_eligible"])
    assert dur.get()[0] == sel["duration_best"]
    for got, name in ((sb, "stamps_best"), (tb, "traj_best"), (db, "dense_best")):
        assert np.array_equal(_bits(got.get()), _bits(sel[name])), name
    # a bound no row meets leaves the outputs about the chosen row alone; `best` may be NULL
    pl.select_retimed_dev(J, lim, -np.inf, 1e-3, 2.0, n_eligible=n.ptr.value, duration_best=dur.ptr.value, traj_best=tb.ptr.value)
    assert int(n.get()[0]) == 0 and dur.get()[0] == sel["duration_best"]
    assert np.array_equal(_bits(tb.get()), _bits(sel["traj_best"]))
    # the bare rule with device pointers
    c = dict(PATH_CASES)["long-D3N20J4"]
    qd, qL, qR, h = rr.path_from_traj(c["traj"], c["dt"], c["J"])
    cap = rr.rate_caps(qd, c["vel"])
    want = engine.retime_path(qd, qL, qR, cap, c["acc"], h, max_rate=MAX_RATE)
    M = qd.shape[0]
    ins = [_DevBuf(x) for x in (qd, qL, qR, cap)]
    po = dict(sdot=_DevBuf(np.zeros(M)), u=_DevBuf(np.zeros(M)), stamps=_DevBuf(np.zeros(M)), duration=_DevBuf(np.zeros(1)),
              status=_DevBuf(np.full(1, -7, dtype=np.int32)), achieved=_DevBuf(np.zeros(4)))
    ws = _DevBuf(np.zeros(3 * M))
    rc = engine.lib.gpmp2mi_retime_path_dev(1, M, 3, *[x.ptr for x in ins], E.dptr(np.ascontiguousarray(c["acc"])), h, MAX_RATE,
                                            -1.0, -1.0, *[po[k].ptr for k in PROFILE], ws.ptr, None)
    assert rc == 0
    _same_bits({k: v.get().reshape(want[k].shape) for k, v in po.items()}, want, PROFILE, what="gpmp2mi_retime_path_dev")
