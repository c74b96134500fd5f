"""The self-collision check on the device (include/gpmp2mi.h "self-collision check") against the CPU oracle's composition
interpolate_traj -> sphere_centers -> pair distances (tests/self_reference.py), through every entry point: caller
buffers and plans; values at every tile edge and every way the spheres and pairs are shared, determinism, non-finite
input, permuted tables, the list rule, selection, and that the existing calls are left alone.

Tolerances are the project's own, as in tests/test_gpu_score.py: costs rtol 1e-8 / atol 1e-12, clearances atol 1e-9."""
import ctypes as C

import numpy as np
import pytest

import score_reference as ref
import self_reference as sr
from gpmp2_amd import engine as E
from gpmp2_amd import scoring

pytestmark = pytest.mark.gpu
FIVE = scoring.SELF_NAMES


def _same_bits(a, b, rows=None, what="", names=FIVE):
    """the outputs agree bit for bit (rows: (rows of a, rows of b))"""
    for k in names:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows[0]], b[k][rows[1]])
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.dtype == np.float64:
            x, y = x.view(np.int64), y.view(np.int64)
        assert np.array_equal(x, y), (what, k, a[k], b[k])


def _check_against_reference(dev, exp, label):
    B = len(exp["invalid"])
    finite = np.isfinite(exp["min_self_clearance"])
    dclr = np.abs(dev["min_self_clearance"][finite] - exp["min_self_clearance"][finite]).max() if finite.any() else 0.0
    print(f"{label}: max |d support| {np.abs(dev['self_support_cost'] - exp['self_support_cost']).max():.2e}, max |d dense| "
          f"{np.abs(dev['self_dense_cost'] - exp['self_dense_cost']).max():.2e}, max |d clearance| {dclr:.2e}, "
          f"gaps {exp['gap']}")
    np.testing.assert_allclose(dev["self_support_cost"], exp["self_support_cost"], rtol=1e-8, atol=1e-12, err_msg=label)
    np.testing.assert_allclose(dev["self_dense_cost"], exp["self_dense_cost"], rtol=1e-8, atol=1e-12, err_msg=label)
    np.testing.assert_allclose(dev["min_self_clearance"], exp["min_self_clearance"], rtol=0, atol=1e-9, err_msg=label)
    assert np.array_equal(dev["invalid"], exp["invalid"]), (label, dev["invalid"], exp["invalid"])
    # worst: the reference's argmin wherever its runner-up is more than 1e-6 above the minimum; a closer row whose
    # (state, pair) differs is excused, at most 10 % of the rows (tests/test_self_cpu.py: the inputs keep to that)
    with np.errstate(invalid="ignore"):
        decided = ~(exp["gap"] <= 1e-6)
    differs = (dev["worst"] != exp["worst"]).any(axis=1)
    assert not (differs & decided).any(), (label, dev["worst"][differs], exp["worst"][differs], exp["gap"][differs])
    assert differs.sum() <= 0.1 * B, (label, "rows excused", int(differs.sum()), B, exp["gap"][differs])


@pytest.fixture(scope="module")
def robots_(engine, oracle):
    """model, device handle and oracle handle per robot of the cases, made once"""
    made = {}

    def get(name):
        if name not in made:
            model = sr.models()[name]()
            made[name] = (model, engine.robot(model), oracle.robot(model))
        return made[name]
    return get


@pytest.mark.parametrize("case", sr.GPU_CASES, ids=[sr.case_id(c) for c in sr.GPU_CASES])
def test_scores_match_the_reference(engine, oracle, robots_, case):
    name, which, (N, J) = case
    model, r, ro = robots_(name)
    table = sr.case_table(name, which, oracle, model, ro)
    traj = sr.case_traj(name, N)
    assert traj.shape[0] == 3
    if which in ("generated", "generated3"):     # the library's list is the reference's list
        pairs = engine.generate_self_pairs(r, 3 if which == "generated3" else 2, np.zeros((1, model.dof())))
        assert np.array_equal(pairs.data, table), (pairs.P, len(table))
    else:
        pairs = engine.self_pairs(r, table)
        assert pairs.P == len(table) and np.array_equal(pairs.data, table)
    exp = sr.oracle_self_score(oracle, model, ro, table, sr.DELTA_T, J, traj)
    dev = engine.self_score_traj(r, pairs, sr.DELTA_T, J, traj)
    _check_against_reference(dev, exp, sr.case_id(case))
    if J == 0:   # the support states are all there is: the two sums are the same additions
        assert np.array_equal(dev["self_dense_cost"].view(np.int64), dev["self_support_cost"].view(np.int64))
    if which == "none":
        assert (dev["self_dense_cost"] == 0.0).all() and np.isposinf(dev["min_self_clearance"]).all()
        assert (dev["worst"] == -1).all() and (dev["invalid"] == 0).all()
    if name == "point2":   # one distance, 5 exactly, in every state: the tie goes to state 0
        assert (dev["min_self_clearance"] == 3.75).all() and (dev["worst"] == 0).all()
    if name == "arm3s":    # row 0 is folded onto itself, row 1 stretched out: the check cannot pass on "all clear"
        assert dev["min_self_clearance"][0] < -0.05 and dev["self_dense_cost"][0] > 0.0
        assert dev["min_self_clearance"][1] > 0.05 and dev["self_dense_cost"][1] == 0.0
    # a row alone, and in another batch at another position: the same bits
    _same_bits(engine.self_score_traj(r, pairs, sr.DELTA_T, J, traj[1]), dev, rows=(0, 1), what="alone vs row 1 of 3")
    other = np.concatenate([traj[2:], traj[:1], traj[1:2], traj[:2]])
    _same_bits(engine.self_score_traj(r, pairs, sr.DELTA_T, J, other), dev, rows=(2, 1), what="row 2 of 5 vs row 1 of 3")
    pairs.close()


def test_table_errors_with_a_live_robot(engine, robots_):
    model, r, _ = robots_("wam")
    lib, out = engine.lib, C.c_void_p()
    for bad in ([[0, 16, 0, 1]], [[16, 0, 0, 1]], [[-1, 2, 0, 1]], [[3, 3, 0, 1]], [[0.5, 2, 0, 1]], [[0, 2, 0, 1], [1, 2.25, 0, 1]]):
        d = np.ascontiguousarray(bad, dtype=np.float64)
        assert lib.gpmp2mi_self_pairs_create(r.ptr, len(d), E.dptr(d), C.byref(out)) == 1, bad
        assert out.value is None
    assert lib.gpmp2mi_self_pairs_generate(r.ptr, 0, 0, None, 0.0, 1.0, C.byref(out)) == 1        # min_joint_gap < 1
    assert lib.gpmp2mi_self_pairs_generate(r.ptr, 2, 1, None, 0.0, 1.0, C.byref(out)) == 1        # n_ref without ref_conf
    assert lib.gpmp2mi_self_pairs_generate(r.ptr, 2, -1, None, 0.0, 1.0, C.byref(out)) == 1
    empty = engine.self_pairs(r, [])                                                               # P = 0 is a table
    assert empty.P == 0 and empty.data.shape == (0, 4)
    assert engine.generate_self_pairs(r, 7).P == 0                                                 # nothing 7 joints apart
    # a table made for another sphere model
    _, r3, _ = robots_("arm3s")
    t = np.zeros((2, 3, 14))
    with pytest.raises(E.Gpmp2miError) as ei:
        engine.self_score_traj(r, engine.self_pairs(r3, [[0, 5, 0, 1]]), 0.1, 1, t)
    assert ei.value.code == 1 and "another robot" in str(ei.value)
    wam_pairs = engine.self_pairs(r, [[0, 15, 0, 1]])
    one = np.zeros(2)
    assert lib.gpmp2mi_self_score_traj(r.ptr, wam_pairs.ptr, 0.1, -1, 2, 2, E.dptr(t), E.dptr(one), None, None, None, None) == 1
    assert lib.gpmp2mi_self_score_traj(r.ptr, wam_pairs.ptr, 0.0, 1, 2, 2, E.dptr(t), E.dptr(one), None, None, None, None) == 1
    assert lib.gpmp2mi_self_score_traj(r.ptr, wam_pairs.ptr, 0.1, 1, -1, 2, E.dptr(t), E.dptr(one), None, None, None, None) == 1
    assert lib.gpmp2mi_self_score_traj(r.ptr, wam_pairs.ptr, 0.1, 1, 2, 0, E.dptr(t), E.dptr(one), None, None, None, None) == 1
    one[:] = 7.0
    assert lib.gpmp2mi_self_score_traj(r.ptr, wam_pairs.ptr, 0.1, 1, 0, 2, E.dptr(t), E.dptr(one), None, None, None, None) == 0   # B = 0
    assert (one == 7.0).all()
    assert lib.gpmp2mi_self_score_traj(r.ptr, wam_pairs.ptr, 0.1, 1, 2, 2, E.dptr(t), None, None, None, None, None) == 0  # all NULL


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
    ro, so = oracle.robot(p.model), ref.oracle_sdf(oracle, p.sdf_origin, p.sdf_cell, p.sdf_data)
    dt = ref.delta_t(p.setting)
    pairs = engine.generate_self_pairs(r, 2, np.zeros((1, 7)))
    return dict(p=p, J=J, r=r, s=s, pl=pl, res=res, dt=dt, pairs=pairs,
                obstacle=ref.oracle_score(oracle, p.model, ro, so, dt, J, res["traj"]),
                self=sr.oracle_self_score(oracle, p.model, ro, pairs.data, dt, J, res["traj"]))


def test_a_row_scores_the_same_bits_alone_in_a_batch_and_through_the_plan(engine, wam16):
    w = wam16
    pl, r, pairs, dt, J, traj = w["pl"], w["r"], w["pairs"], w["dt"], w["J"], w["res"]["traj"]
    assert pairs.P == 78
    through_plan = pl.self_score(pairs, J)
    _check_against_reference(through_plan, w["self"], "wam16 through the plan")
    batch = engine.self_score_traj(r, pairs, dt, J, traj)
    _same_bits(through_plan, batch, what="Plan.self_score vs Engine.self_score_traj on the fetched result")
    _same_bits(batch, engine.self_score_traj(r, pairs, dt, J, traj), what="twice in a row")
    _same_bits(through_plan, pl.self_score(pairs, J), what="Plan.self_score twice in a row")
    _same_bits(engine.self_score_traj(r, pairs, dt, J, traj[11]), batch, rows=(0, 11), what="alone vs row 11 of 16")
    big = np.repeat(traj, 16, axis=0)                    # 256 rows
    _same_bits(engine.self_score_traj(r, pairs, dt, J, big), batch, rows=(11 * 16 + 5, 11), what="in a batch of 256")
    # only the outputs asked for are written; another inter_step grows the workspace and leaves the answers alone
    part = pl.self_score(pairs, J, out={"min_self_clearance": np.zeros(16)})
    assert np.array_equal(part["min_self_clearance"].view(np.int64), through_plan["min_self_clearance"].view(np.int64))
    pl.self_score(pairs, 9)
    _same_bits(through_plan, pl.self_score(pairs, J), what="after the workspace grew")


def test_a_nan_row_is_invalid_everywhere_and_leaves_the_others_alone(engine, wam16):
    w = wam16
    r, pairs, dt, J, traj = w["r"], w["pairs"], w["dt"], w["J"], w["res"]["traj"]
    clean = engine.self_score_traj(r, pairs, dt, J, traj)
    bad = traj.copy()
    bad[3] = np.nan
    sc = engine.self_score_traj(r, pairs, dt, J, bad)
    Md = scoring.checked_states(traj.shape[1] - 1, J)
    assert sc["invalid"][3] == Md * pairs.P and sc["self_dense_cost"][3] == 0.0 and sc["self_support_cost"][3] == 0.0
    assert np.isposinf(sc["min_self_clearance"][3]) and tuple(sc["worst"][3]) == (-1, -1)
    keep = [b for b in range(traj.shape[0]) if b != 3]
    _same_bits(sc, clean, rows=(keep, keep), what="ordinary rows beside a NaN row")
    fe = np.ones(traj.shape[0])
    fe[3] = 0.0                      # the cheapest row by far
    ok = scoring.eligible(fe, None, np.full(len(fe), 1.0), None, 0.0, False, sc["min_self_clearance"], sc["invalid"], -np.inf)
    assert not ok[3] and scoring.select_rule(fe, None, np.full(len(fe), 1.0), None, 0.0, False, sc["min_self_clearance"],
                                             sc["invalid"], -np.inf)[0] != 3
    # one joint of one support state: the states around it are invalid for the pairs behind that joint, no others
    some = traj.copy()
    some[5, 4, 6] = np.inf           # the last joint: only the hand's spheres move with it
    got = engine.self_score_traj(r, pairs, dt, J, some)
    hand = int(((pairs.data[:, 0] >= 10) | (pairs.data[:, 1] >= 10)).sum())
    assert 0 < got["invalid"][5] <= (2 * J + 1) * hand and np.isfinite(got["self_dense_cost"][5])
    _same_bits(got, clean, rows=([0, 4, 6], [0, 4, 6]), what="rows beside a row with one non-finite joint")


def test_permuting_the_table_keeps_the_minimum_and_maps_worst(engine, wam16):
    w = wam16
    r, pairs, dt, J, traj = w["r"], w["pairs"], w["dt"], w["J"], w["res"]["traj"]
    base = engine.self_score_traj(r, pairs, dt, J, traj)
    perm = np.random.default_rng(5).permutation(pairs.P)
    shuffled = engine.self_pairs(r, pairs.data[perm])
    got = engine.self_score_traj(r, shuffled, dt, J, traj)
    assert np.array_equal(got["min_self_clearance"].view(np.int64), base["min_self_clearance"].view(np.int64))
    assert np.array_equal(got["invalid"], base["invalid"])
    assert np.array_equal(got["worst"][:, 0], base["worst"][:, 0])
    assert np.array_equal(perm[got["worst"][:, 1]], base["worst"][:, 1])
    np.testing.assert_allclose(got["self_dense_cost"], base["self_dense_cost"], rtol=1e-8, atol=1e-12)


def test_select_checked_is_the_extended_rule_on_the_reference_scores(engine, wam16):
    w = wam16
    pl, pairs, J, res, ob, se = w["pl"], w["pairs"], w["J"], w["res"], w["obstacle"], w["self"]
    plain = pl.select(J, 0.0, False)
    want = scoring.select_rule(res["final_error"], res["status"], ob["min_clearance"], ob["out_of_range"], 0.0, False,
                               se["min_self_clearance"], se["invalid"], 0.0)
    sel = pl.select_checked(J, pairs, 0.0, False, 0.0)
    print(f"select {plain['best']} of {plain['n_eligible']}, select_checked {sel['best']} of {sel['n_eligible']}, "
          f"reference {want}")
    assert (sel["best"], sel["n_eligible"]) == want
    passing = scoring.eligible(res["final_error"], res["status"], ob["min_clearance"], ob["out_of_range"], 0.0, False)
    hit = int((passing & (se["min_self_clearance"] < 0.0)).sum())
    assert hit == 9 and plain["n_eligible"] - sel["n_eligible"] == hit
    if sel["best"] == plain["best"]:
        assert np.array_equal(sel["traj_best"].view(np.int64), plain["traj_best"].view(np.int64))
        assert np.array_equal(sel["dense_best"].view(np.int64), plain["dense_best"].view(np.int64))
    assert np.array_equal(sel["traj_best"].view(np.int64), res["traj"][want[0]].view(np.int64))
    # the device scores give the same pick as the reference scores, for several thresholds
    dev_ob, dev_se = pl.score(J), pl.self_score(pairs, J)
    for req, rir, req_self in ((0.0, True, 0.0), (-np.inf, False, -np.inf), (0.0, False, 0.02), (0.0, False, -0.05), (0.02, True, 0.01)):
        a = pl.select_checked(J, pairs, req, rir, req_self)
        b = scoring.select_rule(res["final_error"], res["status"], dev_ob["min_clearance"], dev_ob["out_of_range"], req, rir,
                                dev_se["min_self_clearance"], dev_se["invalid"], req_self)
        assert (a["best"], a["n_eligible"]) == b, (req, rir, req_self, a["best"], a["n_eligible"], b)
    # an empty table asks nothing more than select
    empty = engine.self_pairs(w["r"], [])
    a = pl.select_checked(J, empty, 0.0, False, 0.0)
    assert (a["best"], a["n_eligible"]) == (plain["best"], plain["n_eligible"])
    assert np.array_equal(a["dense_best"].view(np.int64), plain["dense_best"].view(np.int64))
    # a threshold no row meets
    none = pl.select_checked(J, pairs, 0.0, False, 10.0)
    assert (none["best"], none["n_eligible"]) == (-1, 0) and none["traj_best"] is None and none["dense_best"] is None


class _DevArray:
    """a device buffer from the library's own HIP runtime (gpmp2mi_debug_device_*): no second runtime in the process"""

    def __init__(self, engine, shape, dtype, fill_byte):
        self.eng, self.host = engine, np.zeros(shape, dtype=dtype)
        self.p = C.c_void_p()
        engine._ck(engine.lib.gpmp2mi_debug_device_alloc(C.c_size_t(self.host.nbytes), fill_byte, C.byref(self.p)))

    @property
    def ptr(self):
        return self.p.value

    def read(self):
        self.eng._ck(self.eng.lib.gpmp2mi_debug_device_read(self.host.ctypes.data_as(C.c_void_p), self.p,
                                                            C.c_size_t(self.host.nbytes)))
        return self.host.copy()

    def free(self):
        self.eng._ck(self.eng.lib.gpmp2mi_debug_device_free(self.p))


def test_the_dev_forms_write_device_buffers_and_leave_them_alone_when_nothing_is_chosen(engine, wam16):
    w = wam16
    pl, pairs, J, p = w["pl"], w["pairs"], w["J"], w["p"]
    N, D, B = p.setting.total_step, p.setting.dof, p.B
    Md = scoring.checked_states(N, J)
    FILL = 0x7B
    best, n = _DevArray(engine, (1,), np.int32, FILL), _DevArray(engine, (1,), np.int32, FILL)
    tb, db = _DevArray(engine, (N + 1, 2 * D), np.float64, FILL), _DevArray(engine, (Md, 2 * D), np.float64, FILL)
    clr, inv, worst = _DevArray(engine, (B,), np.float64, FILL), _DevArray(engine, (B,), np.int32, FILL), _DevArray(engine, (B, 2), np.int32, FILL)
    untouched = tb.read()
    pl.select_checked_dev(J, pairs, 0.0, False, 10.0, best=best.ptr, n_eligible=n.ptr, traj_best=tb.ptr, dense_best=db.ptr)
    pl.self_score_dev(pairs, J, min_self_clearance=clr.ptr, invalid=inv.ptr, worst=worst.ptr)
    host = pl.self_score(pairs, J)                     # waits for the null stream
    assert (int(best.read()[0]), int(n.read()[0])) == (-1, 0)
    assert np.array_equal(tb.read().view(np.int64), untouched.view(np.int64))
    assert (db.read().view(np.int64) == untouched.view(np.int64).reshape(-1)[0]).all()
    assert np.array_equal(clr.read().view(np.int64), host["min_self_clearance"].view(np.int64))
    assert np.array_equal(inv.read(), host["invalid"]) and np.array_equal(worst.read(), host["worst"])
    want = pl.select_checked(J, pairs, 0.0, False, 0.0)
    pl.select_checked_dev(J, pairs, 0.0, False, 0.0, best=best.ptr, n_eligible=n.ptr, traj_best=tb.ptr, dense_best=db.ptr)
    pl.self_score(pairs, J)
    assert (int(best.read()[0]), int(n.read()[0])) == (want["best"], want["n_eligible"])
    assert np.array_equal(tb.read().view(np.int64), want["traj_best"].view(np.int64))
    assert np.array_equal(db.read().view(np.int64), want["dense_best"].view(np.int64))
    for b in (best, n, tb, db, clr, inv, worst):
        b.free()


def test_the_existing_calls_are_left_alone(engine, wam16):
    """plan.score before and after the new calls, and update(1) with and without them in front: array_equal"""
    w = wam16
    p, r, s, pairs, J = w["p"], w["r"], w["s"], w["pairs"], w["J"]
    plans = []
    for with_self in (False, True):
        pl = engine.plan(r, s, p.setting, p.B)
        pl.set_problem(*_args(p), p.init)
        pl.optimize()
        before = pl.score(J)
        sel_before = pl.select(J, 0.0, True)
        if with_self:
            pl.self_score(pairs, J)
            pl.select_checked(J, pairs, 0.0, True, 0.0)
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


def test_plan_states_and_mismatched_tables(engine, wam16, robots_):
    w = wam16
    p, r, s, pairs, J = w["p"], w["r"], w["s"], w["pairs"], w["J"]
    pl = engine.plan(r, s, p.setting, p.B)
    for call in (lambda: pl.self_score(pairs, J), lambda: pl.select_checked(J, pairs)):     # nothing to score yet
        with pytest.raises(E.Gpmp2miError) as ei:
            call()
        assert ei.value.code == 1 and "not been optimized" in str(ei.value)
    pl.set_problem(*_args(p), p.init)
    pl.optimize()
    _, r3, _ = robots_("arm3s")
    other = engine.self_pairs(r3, [[0, 5, 0, 1]])
    for call in (lambda: pl.self_score(other, J), lambda: pl.select_checked(J, other)):
        with pytest.raises(E.Gpmp2miError) as ei:
            call()
        assert ei.value.code == 1 and "another robot" in str(ei.value)
    lib = engine.lib
    assert lib.gpmp2mi_plan_self_score(pl.h.ptr, pairs.ptr, -1, None, None, None, None, None) == 1
    assert lib.gpmp2mi_plan_select_checked(pl.h.ptr, -1, 0.0, 0, pairs.ptr, 0.0, None, None, None, None) == 1
    assert lib.gpmp2mi_plan_self_score(pl.h.ptr, pairs.ptr, J, None, None, None, None, None) == 0     # every output may be NULL
    pl.optimize_queue(*_args(p), p.init)          # a queue run leaves no problem behind
    with pytest.raises(E.Gpmp2miError) as ei:
        pl.self_score(pairs, J)
    assert ei.value.code == 1
    pl.close()
