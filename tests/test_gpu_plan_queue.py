"""A queue of problems through one plan (gpmp2mi_plan_optimize_queue): every queued problem returns exactly what plain
set_problem + optimize runs of it return on the same plan -- value-identical trajectories, final errors and error
traces, identical iteration counts and status codes -- on every solver path, while finished slots are refilled."""
import math

import numpy as np
import pytest

import gpmp2_amd as g
from gpmp2_amd import engine as E
from gpmp2_amd import problems
from test_gpu_robots import _tree_problem, _wide_models

pytestmark = pytest.mark.gpu


def _rows(p):
    return p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init


def _expand(p, M, scale, seed=1234):
    """M copies of a one-problem Problem; problem b >= 1 gets init += A_b sin(pi i / N) on the configuration, as
    problems.wam_restarts perturbs its restarts (A_b ~ N(0, scale^2 I) from default_rng(seed + b))."""
    D, N = p.setting.dof, p.setting.total_step
    rep = lambda a: np.repeat(np.asarray(a)[:1], M, axis=0).copy()
    sc, sv, ec, ev, init = (rep(a) for a in _rows(p))
    bump = np.sin(math.pi * np.arange(N + 1) / N)
    for b in range(1, M):
        A = np.random.default_rng(seed + b).normal(0.0, scale, size=D)
        init[b, :, :D] += bump[:, None] * A[None, :]
    return sc, sv, ec, ev, init


def _plain(pl, rows):
    """set_problem + optimize on chunks of B (the last chunk padded with copies of its last problem); the passes of the
    Gauss-Newton fast path (max(iters) + 1 per chunk) and the busy slot-passes (iters + 1 per problem)"""
    B, M = pl.B, rows[0].shape[0]
    out, passes, busy = [], 0, 0
    for c0 in range(0, M, B):
        idx = list(range(c0, min(c0 + B, M)))
        pad = idx + [idx[-1]] * (B - len(idx))
        pl.set_problem(*[a[pad] for a in rows])
        pl.optimize()
        r = pl.result()
        out.append({k: v[:len(idx)] for k, v in r.items()})
        passes += int(r["iters"].max()) + 1
        busy += int((r["iters"] + 1).sum())
    res = {k: np.concatenate([o[k] for o in out]) for k in out[0]}
    return res, passes, busy


def _assert_same(q, ref):
    assert list(q["iters"]) == list(ref["iters"])
    assert list(q["status"]) == list(ref["status"])
    assert np.array_equal(q["traj"], ref["traj"])
    assert np.array_equal(q["final_error"], ref["final_error"])
    assert np.array_equal(q["error_trace"], ref["error_trace"], equal_nan=True)


def _check(engine, p, rows, B, forms=None):
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pl = engine.plan(r, s, p.setting, B, forms)
    q = pl.optimize_queue(*rows)
    stats = pl.queue_stats()
    ref, passes, busy = _plain(pl, rows)
    _assert_same(q, ref)
    assert stats["slot_passes"] == B * stats["passes"]
    return q, stats, passes, busy, pl


# ------------------------------------------------------------------ the headline graph
def test_headline_wam_restarts_through_64_slots(engine, oracle):
    p = problems.wam_restarts(B=160, opt="GN")
    rows = _rows(p)
    q, st, plain_passes, plain_busy, pl = _check(engine, p, rows, 64)
    assert len(set(q["iters"])) > 1
    assert st["passes"] < plain_passes, (st, plain_passes)
    plain_ratio = plain_busy / (64 * plain_passes)
    assert st["busy_slot_passes"] / st["slot_passes"] > plain_ratio, (st, plain_ratio)
    # against the CPU oracle (SURVEY 8(d) contract): 16 of the problems
    sel = np.arange(0, 160, 10)
    ro, so = oracle.robot(p.model), oracle.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    ref = oracle.batch_optimize(ro, so, p.setting, *[a[sel] for a in rows])
    assert list(q["iters"][sel]) == list(ref["iters"]) and list(q["status"][sel]) == list(ref["status"])
    np.testing.assert_allclose(q["traj"][sel], ref["traj"], atol=1e-6)


# ------------------------------------------------------------------ every form, small graphs, M = 2B + 3
def _wam_small(opt="GN", max_iter=50):
    return problems.wam_restarts(B=11, total_step=16, obs_check_inter=3, opt=opt, sdf="40", max_iter=max_iter)


WAM_FORMS = [("GN", None, 0), ("GN", {"no_fused_finish": 1}, 0), ("GN", {"generic_gn": 1}, 0), ("LM", None, 0),
             ("DOGLEG", None, 0), ("GN", None, 3)]


@pytest.mark.parametrize("opt,forms,fixed", WAM_FORMS, ids=["gn", "gn_no_fused", "gn_generic", "lm", "dogleg", "gn_fixed3"])
def test_wam_forms(engine, opt, forms, fixed):
    p = _wam_small(opt)
    p.setting.fixed_iterations = fixed
    q = _check(engine, p, _rows(p), 4, forms)[0]
    if not fixed:
        assert len(set(q["iters"])) > 1, list(q["iters"])


def _small_cases():
    def arm3():
        p = problems.arm3_planner()
        return p, _expand(p, 9, 0.3), 3
    def point():
        p = problems.point_robot_2d()
        return p, _expand(p, 9, 3.0), 3
    def mobile(opt):
        p = problems.mobile_arm_config5()
        {"GN": p.setting.setGaussNewton, "DOGLEG": p.setting.setDogleg}[opt]()
        return p, _expand(p, 11, 0.3), 4
    def goal():
        p = problems.arm3_goal_reach()
        return p, _expand(p, 9, 0.3), 3
    return {"arm3_planner": arm3, "point_robot_2d": point, "mobile_arm_gn": lambda: mobile("GN"),
            "mobile_arm_dogleg": lambda: mobile("DOGLEG"), "arm3_goal_reach": goal}


@pytest.mark.parametrize("name", ["arm3_planner", "point_robot_2d", "mobile_arm_gn", "mobile_arm_dogleg", "arm3_goal_reach"])
def test_robot_kinds_and_extras(engine, name):
    p, rows, B = _small_cases()[name]()
    q = _check(engine, p, rows, B)[0]
    assert len(set(q["iters"])) > 1, list(q["iters"])


def _spread(p, M, scale, seed=77):
    """M problems of a one-problem tree-robot Problem: straight-line inits from perturbed goals"""
    D, N = p.setting.dof, p.setting.total_step
    rng = np.random.default_rng(seed)
    sc = np.repeat(p.start_conf[:1], M, 0)
    ec = np.repeat(p.end_conf[:1], M, 0) + np.r_[np.zeros((1, D)), scale * rng.normal(size=(M - 1, D))]
    init = np.zeros((M, N + 1, 2 * D))
    for b in range(M):
        for i in range(N + 1):
            init[b, i, :D] = sc[b] * (N - i) / N + ec[b] * i / N
        init[b, :, D:] = (ec[b] - sc[b])[None, :] / 3.0
    z = np.zeros((M, D))
    return sc, z.copy(), ec, z.copy(), init


@pytest.mark.parametrize("forms", [None, {"wide_dense": 1}], ids=["wide", "wide_dense"])
def test_mobile_wam_wide(engine, forms):
    p = _tree_problem(_wide_models()["mobile WAM (dof 10)"], N=10, inter=2, opt="GN")
    q = _check(engine, p, _spread(p, 9, 0.3), 3, forms)[0]
    assert len(set(q["iters"])) > 1, list(q["iters"])


def test_pr2_dense(engine):
    model = g.generateMobileArm("PR2")
    p = _tree_problem(model, N=8, inter=1, opt="GN")
    p.end_conf[0, 3] = 0.2
    p.end_conf[0, 4:] = np.tile(np.linspace(0.2, 0.8, 7), 2) * np.r_[np.ones(7), -np.ones(7)]
    q = _check(engine, p, _spread(p, 7, 0.2), 2)[0]
    assert len(set(q["iters"])) > 1, list(q["iters"])


# ------------------------------------------------------------------ runs longer than one plain run's pass arrays
def test_more_passes_than_max_pass(engine):
    p = problems.wam_restarts(B=40, total_step=16, obs_check_inter=3, opt="GN", sdf="40", max_iter=5)
    q, st, _, _, _ = _check(engine, p, _rows(p), 2)
    assert st["passes"] > 5 + 3, st


# ------------------------------------------------------------------ edge cases
def test_edge_cases(engine):
    p = _wam_small("GN")
    rows = _rows(p)
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pl = engine.plan(r, s, p.setting, 4)
    for M in (3, 1):   # M < B, M = 1
        sub = [a[:M] for a in rows]
        q = pl.optimize_queue(*sub)
        _assert_same(q, _plain(pl, sub)[0])
    a, b = pl.optimize_queue(*rows), pl.optimize_queue(*rows)   # two queue runs in a row
    _assert_same(a, b)
    with pytest.raises(E.Gpmp2miError) as ei:   # the resident problem is gone
        pl.result()
    assert ei.value.code == 1
    # after a queue run, set_problem + optimize equal a fresh plan's results
    four = [x[:4] for x in rows]
    pl.set_problem(*four)
    pl.optimize()
    fresh = engine.plan(r, s, p.setting, 4)
    fresh.set_problem(*four)
    fresh.optimize()
    _assert_same(pl.result(), fresh.result())


class _DevBuf:
    """a device buffer through the HIP runtime (ctypes), for the device-pointer entry points"""
    hip = None

    def __init__(self, a):
        import ctypes
        if _DevBuf.hip is None:
            _DevBuf.hip = ctypes.CDLL("libamdhip64.so")
        self.a = np.ascontiguousarray(a)
        self.ptr = ctypes.c_void_p()
        assert _DevBuf.hip.hipMalloc(ctypes.byref(self.ptr), ctypes.c_size_t(self.a.nbytes)) == 0
        assert _DevBuf.hip.hipMemcpy(self.ptr, self.a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(self.a.nbytes), 1) == 0

    def get(self):
        import ctypes
        out = np.empty_like(self.a)
        assert _DevBuf.hip.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), self.ptr, ctypes.c_size_t(self.a.nbytes), 2) == 0
        return out

    def __del__(self):
        if self.ptr:
            _DevBuf.hip.hipFree(self.ptr)


def test_device_variant(engine):
    """optimize_queue_dev on device buffers and a caller's stream equals the host variant"""
    import ctypes
    p = _wam_small("LM")
    rows = _rows(p)
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pl = engine.plan(r, s, p.setting, 4)
    host = pl.optimize_queue(*rows)
    M, N, D, T = rows[0].shape[0], p.setting.total_step, p.setting.dof, p.setting.max_iter + 1
    ins = [_DevBuf(a) for a in rows]
    outs = dict(traj=_DevBuf(np.zeros((M, N + 1, 2 * D))), iters=_DevBuf(np.zeros(M, np.int32)),
                final_error=_DevBuf(np.zeros(M)), status=_DevBuf(np.zeros(M, np.int32)),
                error_trace=_DevBuf(np.zeros((M, T))))
    stream = ctypes.c_void_p()
    engine._ck(engine.lib.gpmp2mi_debug_stream_create(ctypes.byref(stream)))
    try:
        pl.optimize_queue_dev(M, *[b.ptr.value for b in ins], stream=stream.value,
                              **{k: b.ptr.value for k, b in outs.items()})
    finally:
        engine.lib.gpmp2mi_debug_stream_destroy(stream)
    _assert_same({k: b.get() for k, b in outs.items()}, host)


def test_errors(engine):
    p = _wam_small("GN")
    rows = _rows(p)
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pl = engine.plan(r, s, p.setting, 4)
    lib = engine.lib
    sc = np.ascontiguousarray(rows[0])
    rc = lib.gpmp2mi_plan_optimize_queue(pl.h.ptr, 0, *[E.dptr(np.ascontiguousarray(a)) for a in rows],
                                         None, None, None, None, None)
    assert rc == 1
    pl.fix_state(1, 3, sc[0], np.zeros(p.setting.dof))
    with pytest.raises(E.Gpmp2miError) as ei:
        pl.optimize_queue(*rows)
    assert ei.value.code == 1 and "clear_state_priors" in str(ei.value)
    pl.clear_state_priors(1)
    pl.remove_goal(2)
    with pytest.raises(E.Gpmp2miError) as ei:
        pl.optimize_queue(*rows)
    assert ei.value.code == 1 and "change_goal" in str(ei.value)
    pl.change_goal(2, rows[2][0], rows[3][0])
    _assert_same(pl.optimize_queue(*rows), _plain(pl, rows)[0])
