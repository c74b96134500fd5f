"""The score-and-select stage on the device (include/gpmp2mi.h "scoring") against the CPU oracle's composition
interpolate_traj -> sphere_centers -> sdf_query (tests/score_reference.py), through every entry point: caller buffers,
plans, multi plans; values, determinism, non-finite input, selection, plan states and lifetime.

Tolerances are the project's own: collision costs rtol 1e-8 / atol 1e-12 (tests/test_gpu_planner_api.py), clearances
atol 1e-9 (factor values, tests/test_gpu_factors.py)."""
import ctypes as C
import time

import numpy as np
import pytest

import score_reference as ref
from gpmp2_amd import engine as E
from gpmp2_amd import problems, scoring

pytestmark = pytest.mark.gpu
FIVE = ("support_cost", "dense_cost", "min_clearance", "worst", "out_of_range")
INTER_STEPS = (0, 1, 4, 9)


def _args(p):
    return p.start_conf, p.start_vel, p.end_conf, p.end_vel


def _handles(engine, p):
    return engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)


def _oracle_handles(oracle, p):
    return oracle.robot(p.model), ref.oracle_sdf(oracle, p.sdf_origin, p.sdf_cell, p.sdf_data)


def _same_bits(a, b, rows=None, what=""):
    """the five outputs agree bit for bit (rows: (rows of a, rows of b))"""
    for k in FIVE:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows[0]], b[k][rows[1]])
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.dtype == np.float64:
            x, y = x.view(np.int64), y.view(np.int64)
        assert np.array_equal(x, y), (what, k, a[k], b[k])


def _check_against_oracle(dev, exp, label):
    """the comparisons of one case (all rows of one trajectory batch at one inter_step)"""
    B = len(exp["dense_cost"])
    print(f"{label}: max |d support| {np.abs(dev['support_cost'] - exp['support_cost']).max():.2e}, max |d dense| "
          f"{np.abs(dev['dense_cost'] - exp['dense_cost']).max():.2e}, min gap {np.nanmin(exp['gap']) if B else 0:.2e}, "
          f"out of range {int(exp['out_of_range'].sum())} of {B * exp['pairs']} pairs")
    np.testing.assert_allclose(dev["support_cost"], exp["support_cost"], rtol=1e-8, atol=1e-12, err_msg=label)
    np.testing.assert_allclose(dev["dense_cost"], exp["dense_cost"], rtol=1e-8, atol=1e-12, err_msg=label)
    np.testing.assert_allclose(dev["min_clearance"], exp["min_clearance"], rtol=0, atol=1e-9, err_msg=label)
    # out of range: equal, except for pairs whose oracle centre lies within 1e-9 of a field face (at most 1 % of a row)
    diff = np.abs(dev["out_of_range"].astype(np.int64) - exp["out_of_range"])
    assert (diff <= exp["near_face"]).all() and (diff <= 0.01 * exp["pairs"]).all(), (label, diff, exp["near_face"])
    # worst: the oracle's argmin wherever its runner-up is more than 1e-6 above the minimum (a row without any pair in
    # range counts as decided: (-1, -1)).  A closer row whose (state, sphere) differs is excused -- its value has been
    # compared above -- and at most 10 % of the rows may be; a closer row that agrees needs no excuse (the straight
    # line of config 5 has two coincident spheres, an exact tie in the oracle itself, which the tie rule decides).
    decided = ~(exp["gap"] <= 1e-6)
    differs = (dev["worst"] != exp["worst"]).any(axis=1)
    assert not (differs & decided).any(), (label, dev["worst"][differs], exp["worst"][differs], exp["gap"][differs])
    assert differs.sum() <= 0.1 * B, (label, "rows excused", int(differs.sum()), B, exp["gap"][differs])


@pytest.fixture(scope="module")
def wam32(engine):
    """the solved 32-row WAM batch (N = 20): handles, plan, result"""
    p = problems.wam_restarts(B=32, total_step=20, obs_check_inter=4, sdf="40")
    r, s = _handles(engine, p)
    pl = engine.plan(r, s, p.setting, p.B)
    pl.set_problem(*_args(p), p.init)
    pl.optimize()
    return p, r, s, pl, pl.result()


def _parity_cases():
    wam = ref.motivation_inputs()
    return [("wam16", lambda: wam[0][0]), ("wam32", lambda: wam[1][0]), ("arm3", problems.arm3_planner),
            ("point", problems.point_robot_2d), ("config5", problems.mobile_arm_config5), ("pr2", lambda: ref.pr2_problem(4))]


@pytest.mark.parametrize("name,make", _parity_cases(), ids=[c[0] for c in _parity_cases()])
def test_scores_match_the_oracle_composition(engine, oracle, name, make):
    p = make()
    r, s = _handles(engine, p)
    ro, so = _oracle_handles(oracle, p)
    dt = ref.delta_t(p.setting)
    solved = engine.batch_optimize(r, s, p.setting, *_args(p), p.init)["traj"]
    for which, traj in (("initial", p.init), ("solved", solved)):
        for J in INTER_STEPS:
            dev = engine.score_traj(r, s, dt, J, traj)
            exp = ref.oracle_score(oracle, p.model, ro, so, dt, J, traj)
            _check_against_oracle(dev, exp, f"{name} {which} inter_step={J}")
            if J == 0:   # the support states are all there is: the two sums are the same additions
                assert np.array_equal(dev["dense_cost"].view(np.int64), dev["support_cost"].view(np.int64))
        # the support cost is the value gpmp2mi_collision_cost returns
        cc = engine.collision_cost(r, s, p.setting.total_step, traj)
        for J in INTER_STEPS:
            np.testing.assert_allclose(engine.score_traj(r, s, dt, J, traj)["support_cost"], cc, rtol=1e-8, atol=1e-12)
    if name == "config5":   # most of this robot's spheres are outside its map on the way
        exp = ref.oracle_score(oracle, p.model, ro, so, dt, 4, p.init)
        assert exp["out_of_range"][0] > 0.8 * exp["pairs"]


def test_a_row_scores_the_same_bits_wherever_it_is_scored(engine):
    p = problems.wam_restarts(B=64, total_step=20, obs_check_inter=4, sdf="40")
    r, s = _handles(engine, p)
    dt, J = ref.delta_t(p.setting), 5
    pl = engine.plan(r, s, p.setting, p.B)
    pl.set_problem(*_args(p), p.init)
    pl.optimize()
    traj = pl.result()["traj"]
    through_plan = pl.score(J)
    batch = engine.score_traj(r, s, dt, J, traj)
    again = engine.score_traj(r, s, dt, J, traj)
    alone = engine.score_traj(r, s, dt, J, traj[37])
    _same_bits(through_plan, batch, what="Plan.score vs Engine.score_traj on the fetched result")
    _same_bits(batch, again, what="twice in a row")
    _same_bits(through_plan, pl.score(J), what="Plan.score twice in a row")
    _same_bits(alone, batch, rows=(0, 37), what="alone vs row 37 of 64")
    # and in another batch, at another position
    other = np.concatenate([traj[40:], traj[37:38], traj[:5]])
    _same_bits(engine.score_traj(r, s, dt, J, other), batch, rows=(24, 37), what="row 24 of 30 vs row 37 of 64")
    big = np.repeat(traj, 16, axis=0)                    # 1 024 rows
    sc = engine.score_traj(r, s, dt, J, big)
    _same_bits(sc, batch, rows=(37 * 16 + 5, 37), what="in a batch of 1 024")
    pl.close()


def test_non_finite_rows_are_out_of_range_and_leave_the_others_alone(engine, wam32):
    p, r, s, pl, res = wam32
    dt, J, S = ref.delta_t(p.setting), 4, r.S
    clean = engine.score_traj(r, s, dt, J, res["traj"])
    bad = res["traj"].copy()
    bad[3, 7, 2] = np.nan          # joint 2 of support state 7
    bad[9, 0, 0] = np.inf          # joint 0 of support state 0: sin(inf) is NaN, every centre of that state is
    sc = engine.score_traj(r, s, dt, J, bad)
    keep = [b for b in range(p.B) if b not in (3, 9)]
    _same_bits(sc, clean, rows=(keep, keep), what="ordinary rows beside non-finite ones")
    # row 3: state 7 and the interpolated states on both sides of it are affected from link 2 on; row 9: the states of
    # the first interval, every sphere
    first = int(np.flatnonzero(np.asarray(p.model.flat()["sphere_link"]) >= 2).size)
    assert sc["out_of_range"][3] >= first * (2 * J + 1) and sc["out_of_range"][3] - clean["out_of_range"][3] <= S * (2 * J + 1)
    assert sc["out_of_range"][9] >= S * (J + 1) and sc["out_of_range"][9] - clean["out_of_range"][9] <= S * (J + 1)
    assert np.isfinite(sc["dense_cost"]).all() and not np.isnan(sc["min_clearance"]).any()
    fe = np.zeros(p.B)
    fe[[3, 9]] = -1.0               # the cheapest rows by far
    assert engine.select_best(fe, None, sc["min_clearance"], sc["out_of_range"], -np.inf, True)[0] not in (3, 9)
    # point robot: a coordinate far outside any field
    q = problems.point_robot_2d()
    rq, sq = _handles(engine, q)
    rows = np.repeat(q.init, 3, axis=0)
    rows[1, 4, 0] = 1e300
    ok, got = engine.score_traj(rq, sq, ref.delta_t(q.setting), J, q.init), engine.score_traj(rq, sq, ref.delta_t(q.setting), J, rows)
    _same_bits(got, ok, rows=(0, 0))
    _same_bits(got, ok, rows=(2, 0))
    assert got["out_of_range"][1] >= 1 and np.isfinite(got["dense_cost"][1])
    assert engine.select_best(np.array([2.0, 1.0, 2.0]), None, got["min_clearance"], got["out_of_range"], -np.inf, True)[0] == 0


def test_plan_select_is_the_rule_on_the_device_scores(engine, wam32):
    p, r, s, pl, res = wam32
    dt, J = ref.delta_t(p.setting), 5
    sc = pl.score(J)
    for req, rir in ((0.0, False), (0.0, True), (-np.inf, False), (0.02, True), (10.0, False)):
        sel = pl.select(J, req, rir)
        want = scoring.select_rule(res["final_error"], res["status"], sc["min_clearance"], sc["out_of_range"], req, rir)
        assert (sel["best"], sel["n_eligible"]) == want, (req, rir, sel["best"], sel["n_eligible"], want)
        if want[0] < 0:
            assert sel["traj_best"] is None and sel["dense_best"] is None
            continue
        assert np.array_equal(sel["traj_best"].view(np.int64), res["traj"][want[0]].view(np.int64))
        up = engine.interpolate_traj(p.setting.dof, False, None, dt, J, res["traj"][want[0]][None])[0]
        assert np.array_equal(sel["dense_best"].view(np.int64), up.view(np.int64)), np.abs(sel["dense_best"] - up).max()
    assert pl.select(J, 10.0, False)["n_eligible"] == 0
    # a support-clean, dense-dirty row made the cheapest: skipped at required_clearance = 0, taken at -inf
    dirty = np.flatnonzero((sc["support_cost"] == 0.0) & (sc["dense_cost"] > 0.0))
    assert dirty.size > 0, "the dense check finds nothing the support check misses on this batch"
    fe = res["final_error"].copy()
    fe[dirty[0]] = 0.5 * fe.min()
    assert engine.select_best(fe, res["status"], sc["min_clearance"], sc["out_of_range"], 0.0)[0] != dirty[0]
    assert engine.select_best(fe, res["status"], sc["min_clearance"], sc["out_of_range"], -np.inf)[0] == dirty[0]


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

    def write(self, a):
        a = np.ascontiguousarray(a, dtype=self.host.dtype).reshape(self.host.shape)
        self.eng._ck(self.eng.lib.gpmp2mi_debug_device_write(self.p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes)))

    def free(self):
        self.eng._ck(self.eng.lib.gpmp2mi_debug_device_free(self.p))


def test_select_dev_returns_while_its_stream_is_parked(engine):
    """select_dev / score_dev with device outputs on a stream parked by the stall hook: the calls return while the stream
    is still parked (the outputs still hold their fill pattern), and after the release they hold what the host form
    returns.  One parked episode, bounded by the hook's max_ms."""
    p = problems.wam_restarts(B=32, total_step=20, obs_check_inter=4, sdf="40")
    r, s = _handles(engine, p)
    pl = engine.plan(r, s, p.setting, p.B)
    pl.set_problem(*_args(p), p.init)
    pl.optimize()
    res, lib = pl.result(), engine.lib
    J, N, D = 5, p.setting.total_step, p.setting.dof
    want = pl.select(J, 0.0, True)                # host form; the plan's scoring workspace exists from here on
    assert want["best"] >= 0
    FILL = 0x7B
    sentinel = int(np.frombuffer(bytes([FILL] * 4), dtype=np.int32)[0])
    best, n = _DevArray(engine, (1,), np.int32, FILL), _DevArray(engine, (1,), np.int32, FILL)
    tb = _DevArray(engine, (N + 1, 2 * D), np.float64, FILL)
    db = _DevArray(engine, (scoring.checked_states(N, J), 2 * D), np.float64, FILL)
    sup = _DevArray(engine, (p.B,), np.float64, FILL)
    clr, oor = _DevArray(engine, (p.B,), np.float64, FILL), _DevArray(engine, (p.B,), np.int32, FILL)
    fe, stt = _DevArray(engine, (p.B,), np.float64, 0), _DevArray(engine, (p.B,), np.int32, 0)
    fe.write(res["final_error"])
    stt.write(res["status"])
    bufs = (best, n, tb, db, sup, clr, oor, fe, stt)
    st, tok = C.c_void_p(), C.c_void_p()
    engine._ck(lib.gpmp2mi_debug_stream_create(C.byref(st)))
    engine._ck(lib.gpmp2mi_debug_stall_begin(st, 3000, C.byref(tok)))     # parks the stream, 3 s at the most
    try:
        t0 = time.perf_counter()
        pl.select_dev(J, 0.0, True, best=best.ptr, n_eligible=n.ptr, traj_best=tb.ptr, dense_best=db.ptr, stream=st.value)
        pl.score_dev(J, support_cost=sup.ptr, min_clearance=clr.ptr, out_of_range=oor.ptr, stream=st.value)
        took = time.perf_counter() - t0
        parked = int(best.read()[0]), int(n.read()[0])    # the default stream does not wait for the parked one
    finally:
        engine._ck(lib.gpmp2mi_debug_stall_release(tok))  # releases the stall and waits for that stream
    assert took < 1.0 and parked == (sentinel, sentinel), ("the call waited for its stream", took, parked)
    assert (int(best.read()[0]), int(n.read()[0])) == (want["best"], want["n_eligible"])
    assert np.array_equal(tb.read().view(np.int64), want["traj_best"].view(np.int64))
    assert np.array_equal(db.read().view(np.int64), want["dense_best"].view(np.int64))
    sc = pl.score(J)
    assert np.array_equal(sup.read().view(np.int64), sc["support_cost"].view(np.int64))
    assert np.array_equal(clr.read().view(np.int64), sc["min_clearance"].view(np.int64))
    assert np.array_equal(oor.read(), sc["out_of_range"])
    # gpmp2mi_select_best_dev on the device scores: the same pick
    engine._ck(lib.gpmp2mi_select_best_dev(p.B, fe.ptr, stt.ptr, clr.ptr, oor.ptr, 0.0, 1, best.ptr, n.ptr, st.value))
    pl.score_dev(J, stream=st.value)                      # plan work behind it on the same stream ...
    pl.close()                                            # ... which the plan's destroy waits for
    assert (int(best.read()[0]), int(n.read()[0])) == (want["best"], want["n_eligible"])
    for b in bufs:
        b.free()
    print(f"select_dev + score_dev returned after {took * 1e3:.3f} ms with their stream parked")


def test_select_dev_refuses_misshaped_tensors():
    """torch tensors handed to select_dev are checked before the library is called (no GPU touched: meta-free fake)"""
    class Fake:
        dtype, device = "torch.float64", type("d", (), {"type": "cuda"})()

        def __init__(self, shape):
            self.shape = shape

        def is_contiguous(self):
            return True

        def data_ptr(self):
            raise AssertionError("a mis-shaped tensor was accepted")

    pl = E.Plan.__new__(E.Plan)
    pl.eng, pl.B, pl.N, pl.D = None, 4, 20, 7
    with pytest.raises(ValueError):
        pl.select_dev(5, traj_best=Fake((3, 14)))
    with pytest.raises(ValueError):
        pl.score_dev(5, support_cost=Fake((5,)))


def test_select_of_a_pose2_robot_up_samples_with_the_lie_interpolator(engine):
    """dense_best of a Pose2 robot (config 5) is gpmp2mi_interpolate_traj with lie = 1 of the chosen row: within the
    project's interpolation tolerance (atol 1e-12, tests/test_gpu_factors.py); printed: whether the bits agree too"""
    p = problems.mobile_arm_config5()
    r, s = _handles(engine, p)
    dt = ref.delta_t(p.setting)
    pl = engine.plan(r, s, p.setting, p.B)
    pl.set_problem(*_args(p), p.init)
    pl.optimize()
    traj = pl.result()["traj"]
    for J in (1, 4, 9):
        sel = pl.select(J, -np.inf, False)
        assert (sel["best"], sel["n_eligible"]) == (0, 1)
        up = engine.interpolate_traj(p.setting.dof, True, None, dt, J, traj)[0]
        print(f"config5 inter_step={J}: max |dense_best - interpolate_traj| {np.abs(sel['dense_best'] - up).max():.2e}, "
              f"bitwise {np.array_equal(sel['dense_best'].view(np.int64), up.view(np.int64))}")
        np.testing.assert_allclose(sel["dense_best"], up, rtol=0, atol=1e-12)
        assert np.array_equal(sel["traj_best"].view(np.int64), traj[0].view(np.int64))
    pl.close()


def test_plan_states_and_argument_errors(engine):
    p = problems.wam_restarts(B=6, total_step=12, obs_check_inter=3, sdf="40")
    r, s = _handles(engine, p)
    lib = engine.lib
    dt, J = ref.delta_t(p.setting), 3
    t = np.ascontiguousarray(p.init)
    out = np.zeros(p.B)

    def code(rc):
        assert len(lib.gpmp2mi_last_error()) > 0 or rc == 0
        return rc
    # live handles, bad numbers: refused with ERR_INVALID
    assert code(lib.gpmp2mi_score_traj(r.ptr, s.ptr, dt, -1, p.B, 12, E.dptr(t), E.dptr(out), None, None, None, None)) == 1
    assert code(lib.gpmp2mi_score_traj(r.ptr, s.ptr, dt, J, p.B, 0, E.dptr(t), E.dptr(out), None, None, None, None)) == 1
    assert code(lib.gpmp2mi_score_traj(r.ptr, s.ptr, 0.0, J, p.B, 12, E.dptr(t), E.dptr(out), None, None, None, None)) == 1
    assert code(lib.gpmp2mi_score_traj(r.ptr, s.ptr, dt, J, -1, 12, E.dptr(t), E.dptr(out), None, None, None, None)) == 1
    assert code(lib.gpmp2mi_score_traj(r.ptr, s.ptr, dt, J, p.B, 12, None, E.dptr(out), None, None, None, None)) == 1
    out[:] = 7.0
    assert lib.gpmp2mi_score_traj(r.ptr, s.ptr, dt, J, 0, 12, E.dptr(t), E.dptr(out), None, None, None, None) == 0   # B = 0
    assert (out == 7.0).all()
    pl = engine.plan(r, s, p.setting, p.B)
    for call in (lambda: pl.score(J), lambda: pl.select(J)):           # nothing to score yet
        with pytest.raises(E.Gpmp2miError) as ei:
            call()
        assert ei.value.code == 1 and "not been optimized" in str(ei.value)
    pl.set_problem(*_args(p), p.init)
    with pytest.raises(E.Gpmp2miError) as ei:
        pl.score(J)
    assert ei.value.code == 1
    pl.optimize()
    solved = pl.score(J)
    assert lib.gpmp2mi_plan_score(pl.h.ptr, -1, E.dptr(out), None, None, None, None) == 1
    assert lib.gpmp2mi_plan_select(pl.h.ptr, -1, 0.0, 0, None, None, None, None) == 1
    assert lib.gpmp2mi_plan_score(pl.h.ptr, J, None, None, None, None, None) == 0        # every output may be NULL
    pl.update(1)                                                          # valid after update()
    after = pl.score(J)
    np.testing.assert_allclose(after["support_cost"], engine.collision_cost(r, s, 12, pl.result()["traj"]), rtol=1e-8, atol=1e-12)
    _same_bits(after, engine.score_traj(r, s, dt, J, pl.result()["traj"]), what="after update")
    # a queue run leaves no problem behind; its output rows score like the same problems solved by set_problem + optimize
    q = pl.optimize_queue(*_args(p), p.init)
    for call in (lambda: pl.score(J), lambda: pl.select(J)):
        with pytest.raises(E.Gpmp2miError) as ei:
            call()
        assert ei.value.code == 1
    _same_bits(engine.score_traj(r, s, dt, J, q["traj"]), solved, what="queue rows vs the plan's own result")
    pl.set_problem(*_args(p), p.init)
    pl.optimize()
    _same_bits(pl.score(J), solved, what="solved again")
    pl.close()


def _multi_case(engine, devices):
    p = problems.wam_restarts(B=32, total_step=20, obs_check_inter=4, sdf="40")
    r, s = _handles(engine, p)
    J = 5
    pl = engine.plan(r, s, p.setting, p.B)
    pl.set_problem(*_args(p), p.init)
    pl.optimize()
    one, res = pl.score(J), pl.result()
    mp = engine.multi_plan(r, s, p.setting, p.B, devices)
    with pytest.raises(E.Gpmp2miError) as ei:
        mp.score(J)
    assert ei.value.code == 1
    mp.set_problem(*_args(p), p.init)
    mp.optimize()
    assert np.array_equal(mp.result()["traj"], res["traj"])
    _same_bits(mp.score(J), one, what=f"multi plan {devices} vs one plan")
    for req, rir in ((0.0, True), (-np.inf, False), (10.0, False)):
        a, b = mp.select(J, req, rir), pl.select(J, req, rir)
        assert (a["best"], a["n_eligible"]) == (b["best"], b["n_eligible"]), (req, rir)
        if b["best"] >= 0:
            assert np.array_equal(a["traj_best"].view(np.int64), b["traj_best"].view(np.int64))
            assert np.array_equal(a["dense_best"].view(np.int64), b["dense_best"].view(np.int64))
        else:
            assert a["traj_best"] is None
    assert engine.lib.gpmp2mi_multi_plan_score(mp.h.ptr, -1, None, None, None, None, None) == 1
    assert engine.lib.gpmp2mi_multi_plan_select(mp.h.ptr, -1, 0.0, 0, None, None, None, None) == 1
    mp.close()
    pl.close()


def test_multi_plan_scores_and_selects_like_one_plan(engine):
    _multi_case(engine, [0, 0])
    _multi_case(engine, [0, 0, 0])      # uneven shards (11, 11, 10)


def test_multi_plan_on_two_gpus(engine):
    if engine.device_count() < 2:
        pytest.skip("needs two GPUs")
    _multi_case(engine, [0, 1])


def _counts(engine):
    """what live plans hold (gpmp2mi_debug_resource_counts; the pools may keep more or less after a close)"""
    v = [C.c_long() for _ in range(5)]
    assert engine.lib.gpmp2mi_debug_resource_counts(*[C.byref(x) for x in v]) == 0
    return dict(live_chunks=v[0].value, live_flagbufs=v[2].value, leaked_plans=v[4].value)


def test_scoring_workspace_goes_with_the_plan(engine):
    p = problems.wam_restarts(B=4, total_step=20, obs_check_inter=3, sdf="40")
    r, s = _handles(engine, p)
    engine.plan(r, s, p.setting, p.B).close()            # fills the pools
    base = _counts(engine)
    reps = engine.replica_counts()
    pl = engine.plan(r, s, p.setting, p.B)
    pl.set_problem(*_args(p), p.init)
    pl.optimize()
    live = _counts(engine)
    a = pl.score(2)
    pl.score(9)                                           # a larger workspace replaces the first
    pl.select(9)
    _same_bits(pl.score(2), a, what="after the workspace grew")
    assert _counts(engine) == live                        # the workspace is no arena chunk and no flag buffer
    pl.close()
    assert _counts(engine) == base
    mp = engine.multi_plan(r, s, p.setting, p.B, [0, 0], replicate_all=True)
    mp.set_problem(*_args(p), p.init)
    mp.optimize()
    _same_bits(mp.score(2), a, what="multi plan with copies of the robot and the field")
    mp.select(2)
    mp.close()
    assert _counts(engine) == base and engine.replica_counts() == reps
