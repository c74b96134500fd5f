"""The Python binding of the check stages and selections against include/gpmp2mi.h, without the library: a stand-in for
eng.lib records every call and writes each argument's position through the pointer it was given, so an argument in the
wrong place, or an output array returned under the wrong name, shows on the host.  No GPU, no library, no process."""
import ctypes as C

import numpy as np
import pytest

from gpmp2_amd import engine
from gpmp2_amd.settings import TrajOptimizerSetting
from test_stage_table_cpu import header_params

B, N, D, J = 2, 2, 2, 1
MD = N * (J + 1) + 1
LP_DOUBLE, LP_INT = C.POINTER(C.c_double), C.POINTER(C.c_int)


class Addr(int):
    """a fake device address or stream: arrives as a c_void_p of that value"""


class FakeLib:
    """every attribute is a C function that records (name, args), writes each argument's position into element 0 of a
    typed pointer and into the value behind a byref (unless write = False), and succeeds"""

    def __init__(self, write=True):
        self.calls, self.write = [], write

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            for k, a in enumerate(args if self.write else ()):
                if isinstance(a, (LP_DOUBLE, LP_INT)):
                    if a:
                        a[0] = k
                elif hasattr(getattr(a, "_obj", None), "value"):
                    a._obj.value = k
            return 0
        return fn


class Stub:
    def __init__(self, ptr):
        self.ptr, self.dof, self.L, self.S = ptr, D, D, 3


def dyadic():
    k = 0
    while True:
        k += 1
        yield 0.125 * k


def addresses(names, first=0x10000):
    return {n: Addr(first + 0x1000 * k) for k, n in enumerate(names)}


@pytest.fixture()
def world():
    eng = engine.Engine.__new__(engine.Engine)
    eng.lib = FakeLib()
    setting = TrajOptimizerSetting(D)
    setting.total_step = N
    pl = engine.Plan(eng, Stub(0x100), Stub(0x200), setting, B)
    assert (pl.B, pl.N, pl.D) == (B, N, D)
    return eng, pl


def arrived(arg, value):
    if isinstance(value, engine.MotionLimits):
        return arg._obj is value.c
    if hasattr(value, "ptr"):
        return arg == value.ptr
    if isinstance(value, np.ndarray):
        return C.cast(arg, C.c_void_p).value == value.ctypes.data
    if isinstance(value, Addr):
        return isinstance(arg, C.c_void_p) and arg.value == int(value)
    if isinstance(value, bool):
        return arg == int(value) and not isinstance(arg, bool)
    return type(arg) is type(value) and arg == value


def check(eng, fn, kw, result=None, handle=None):
    """the last recorded call is `fn` with the header's argument count, every keyword that the header names at its
    position, and every value of `result` carrying the position of the header parameter of its name"""
    name, args = eng.lib.calls[-1]
    pars = [p for _, p in header_params(fn)]
    assert name == fn and len(args) == len(pars), (name, len(args), len(pars))
    if handle is not None:
        assert args[0] is handle.ptr
    hits = [k for k in kw if k in pars]
    for k in hits:
        assert arrived(args[pars.index(k)], kw[k]), (fn, k, args[pars.index(k)], kw[k])
    for k, v in (result or {}).items():
        assert k in pars, (fn, k)
        first = v.flat[0] if isinstance(v, np.ndarray) else v
        assert first == pars.index(k), (fn, k, first, pars.index(k))
    return hits


def thresholds(*names):
    d = dyadic()
    return {n: next(d) for n in names}


def stage_inputs():
    return dict(score={}, moving={}, path={}, self=dict(pairs=Stub(0x300)),
                motion=dict(limits=engine.MotionLimits(D, vel=1.0)), torque=dict(dynamics=Stub(0x400)),
                retime=dict(limits=engine.MotionLimits(D, vel=1.0), **thresholds("max_rate", "rate_start", "rate_end")))


STAGE_OUTPUTS = dict(
    score=("support_cost", "dense_cost", "min_clearance", "worst", "out_of_range"),
    self=("self_support_cost", "self_dense_cost", "min_self_clearance", "worst", "invalid"),
    moving=("moving_support_cost", "moving_dense_cost", "min_moving_clearance", "worst", "invalid"),
    path=("max_pos_dev", "max_rot_dev", "worst", "support_cost", "dense_cost", "invalid"),
    motion=("pos_margin", "vel_ratio", "acc_ratio", "point_speed", "time_scale", "worst", "invalid"),
    torque=("torque_ratio", "static_ratio", "torque_time_scale", "worst", "invalid", "tau"),
    retime=("sdot", "u", "stamps", "duration", "status", "achieved", "dense_retimed"))
PLAN_METHOD = dict(score="score", self="self_score", moving="moving_score", path="path_score", motion="motion_score",
                   torque="torque_score", retime="retime")


@pytest.mark.parametrize("key", list(STAGE_OUTPUTS))
def test_plan_stages_host_and_dev(world, key):
    eng, pl = world
    kw = dict(stage_inputs()[key], inter_step=J)
    fn = "gpmp2mi_plan_" + PLAN_METHOD[key]
    o = getattr(pl, PLAN_METHOD[key])(**kw)
    assert tuple(o) == STAGE_OUTPUTS[key] and all(isinstance(v, np.ndarray) for v in o.values())
    assert len(check(eng, fn, kw, o, pl.h)) == len(kw)
    mine = {n: np.zeros_like(v) for n, v in o.items()}               # the caller's arrays are the ones filled
    o2 = getattr(pl, PLAN_METHOD[key])(out=mine, **kw)
    assert all(o2[n] is mine[n] for n in mine)
    check(eng, fn, kw, o2, pl.h)
    dev = dict(kw, stream=Addr(0x7000), **addresses(STAGE_OUTPUTS[key]))
    assert getattr(pl, PLAN_METHOD[key] + "_dev")(**dev) is None
    assert len(check(eng, fn + "_dev", dev, handle=pl.h)) == len(dev)


def selection_cases():
    lim, dyn, pairs = engine.MotionLimits(D, vel=1.0), Stub(0x400), Stub(0x300)
    base = ("required_clearance",)
    return dict(
        select=("gpmp2mi_plan_select", thresholds(*base), None, None),
        select_checked=("gpmp2mi_plan_select_checked", dict(thresholds(*base, "required_self_clearance"), pairs=pairs),
                        None, None),
        select_feasible=("gpmp2mi_plan_select_feasible",
                         dict(thresholds(*base, "required_self_clearance", "required_pos_margin", "max_time_scale"),
                              pairs=pairs, limits=lim), "time_scale_best", None),
        select_dynamic=("gpmp2mi_plan_select_dynamic",
                        dict(thresholds(*base, "required_self_clearance", "required_pos_margin", "max_time_scale"),
                             pairs=pairs, limits=lim, dynamics=dyn), "time_scale_best", ("tau_best", (MD, D))),
        select_retimed=("gpmp2mi_plan_select_retimed",
                        dict(thresholds(*base, "required_self_clearance", "required_pos_margin", "max_duration", "max_rate",
                                        "rate_start", "rate_end"), pairs=pairs, limits=lim),
                        "duration_best", ("stamps_best", (MD,))),
        select_moving=("gpmp2mi_plan_select_moving",
                       dict(thresholds(*base, "required_self_clearance", "required_moving_clearance"), pairs=pairs),
                       None, None),
        select_path=("gpmp2mi_plan_select_path", thresholds(*base, "max_pos_dev_allowed", "max_rot_dev_allowed"),
                     None, None))


@pytest.mark.parametrize("method", list(selection_cases()))
def test_selections_host_and_dev(world, method):
    eng, pl = world
    fn, kw, scalar, row = selection_cases()[method]
    kw = dict(kw, inter_step=J, require_in_range=True)
    extras = ([] if scalar is None else [scalar]) + ([] if row is None else [row[0]])
    keys = ["best", "n_eligible"] + extras + ["traj_best", "dense_best"]
    res = getattr(pl, method)(**kw)
    assert list(res) == keys and type(res["best"]) is int and type(res["n_eligible"]) is int
    assert res["traj_best"].shape == (N + 1, 2 * D) and res["dense_best"].shape == (MD, 2 * D)
    assert scalar is None or type(res[scalar]) is float
    assert row is None or (res[row[0]].shape == row[1] and res[row[0]].dtype == np.float64)
    assert len(check(eng, fn, kw, res, pl.h)) == len(kw)
    dev = dict(kw, stream=Addr(0x7000), **addresses(keys))
    assert getattr(pl, method + "_dev")(**dev) is None
    assert len(check(eng, fn + "_dev", dev, handle=pl.h)) == len(dev)
    # a library that chooses no row: everything about the chosen row is None
    eng.lib = FakeLib(write=False)
    res = getattr(pl, method)(**kw)
    assert list(res) == keys and res["best"] == -1 and res["n_eligible"] == 0
    assert all(res[k] is None for k in keys[2:])


def test_pairs_none_is_a_null_pointer(world):
    eng, pl = world
    lim = engine.MotionLimits(D)
    for method, extra in (("select_feasible", dict(limits=lim)), ("select_dynamic", dict(limits=lim, dynamics=Stub(0x400))),
                          ("select_retimed", dict(limits=lim)), ("select_moving", {}), ("select_distinct", dict(radius=0.5))):
        for suffix in ("", "_dev"):
            getattr(pl, method + suffix)(inter_step=J, pairs=None, **extra)
            name, args = eng.lib.calls[-1]
            pars = [p for _, p in header_params(name)]
            assert name == "gpmp2mi_plan_" + method + suffix and args[pars.index("pairs")] is None


def test_select_distinct_host_and_dev(world):
    eng, pl = world
    w = np.array([0.5, 2.0])
    kw = dict(thresholds("required_clearance", "required_self_clearance", "radius"), inter_step=J, require_in_range=True,
              pairs=Stub(0x300), max_alt=3, weights=w, metric=1)
    res = pl.select_distinct(**kw)
    keys = ["n_modes", "n_eligible", "alt", "alt_size", "alt_error", "mode", "traj_alt", "dense_alt"]
    assert list(res) == keys
    assert res["traj_alt"].shape == (3, N + 1, 2 * D) and res["dense_alt"].shape == (3, MD, 2 * D) and res["mode"].shape == (B,)
    assert len(check(eng, "gpmp2mi_plan_select_distinct", kw, res, pl.h)) == len(kw)
    dev = dict(kw, stream=Addr(0x7000), **addresses(keys))
    pl.select_distinct_dev(**dev)
    assert len(check(eng, "gpmp2mi_plan_select_distinct_dev", dev, handle=pl.h)) == len(dev)


def traj_cases():
    rob, traj = Stub(0x100), np.zeros((B, N + 1, 2 * D))
    lim = engine.MotionLimits(D, vel=1.0)
    common = dict(robot=rob, delta_t=0.25, inter_step=J, traj=traj)
    return dict(
        score=("score_traj", "gpmp2mi_score_traj", dict(common, sdf=Stub(0x200))),
        self=("self_score_traj", "gpmp2mi_self_score_traj", dict(common, pairs=Stub(0x300))),
        motion=("motion_score_traj", "gpmp2mi_motion_score_traj", dict(common, limits=lim)),
        torque=("torque_score_traj", "gpmp2mi_torque_score_traj", dict(common, dynamics=Stub(0x400))),
        retime=("retime_traj", "gpmp2mi_retime_traj",
                dict(common, limits=lim, max_rate=0.5, rate_start=0.375, rate_end=0.625)),
        moving=("moving_score_traj", "gpmp2mi_moving_score_traj",
                dict(common, radius=np.ones(2), centers=np.zeros((2, N + 1, 3)), epsilon=0.125)),
        path=("path_score_traj", "gpmp2mi_path_score_traj",
              dict(common, mode=2, link=1, des=np.zeros((N + 1, 4, 4)), sigma=np.ones(N + 1))))


@pytest.mark.parametrize("key", list(STAGE_OUTPUTS))
def test_engine_traj_calls(world, key):
    eng, _ = world
    method, fn, kw = traj_cases()[key]
    o = getattr(eng, method)(**kw)
    assert tuple(o) == STAGE_OUTPUTS[key]
    assert len(check(eng, fn, kw, o)) == len(kw)
    _, args = eng.lib.calls[-1]
    pars = [p for _, p in header_params(fn)]
    assert args[pars.index("B")] == B and args[pars.index("total_step")] == N
    if key == "moving":
        assert args[pars.index("K")] == 2


def test_torque_without_tau_passes_null(world):
    eng, pl = world
    _, fn, kw = traj_cases()["torque"]
    for call, name in ((lambda: eng.torque_score_traj(tau=False, **kw), fn),
                       (lambda: pl.torque_score(Stub(0x400), J, tau=False), "gpmp2mi_plan_torque_score")):
        o = call()
        assert tuple(o) == STAGE_OUTPUTS["torque"] and o["tau"] is None
        assert eng.lib.calls[-1][0] == name and eng.lib.calls[-1][1][-1] is None
        assert len(eng.lib.calls[-1][1]) == len(header_params(name))


def test_retime_path(world):
    eng, _ = world
    q = np.zeros((B, MD, D))
    kw = dict(qd=q, qdd_left=q.copy(), qdd_right=q.copy(), cap=np.ones((B, MD)), acc=np.ones(D), h=0.125, max_rate=0.25,
              rate_start=0.375, rate_end=0.5)
    o = eng.retime_path(**kw)
    assert tuple(o) == STAGE_OUTPUTS["retime"][:-1] and o["stamps"].shape == (B, MD) and o["achieved"].shape == (B, 4)
    assert len(check(eng, "gpmp2mi_retime_path", kw, o)) == len(kw)
    args = eng.lib.calls[-1][1]
    assert args[:3] == (B, MD, D)
    eng.retime_path(q, q, q, np.ones((B, MD)), None, 0.125)                 # free ends are -1
    assert eng.lib.calls[-1][1][10:12] == (-1.0, -1.0)


def test_multi_plan_score_and_select(world):
    eng, pl = world
    mp = engine.MultiPlan(eng, Stub(0x100), Stub(0x200), pl.setting, B, [0, 0])
    o = mp.score(inter_step=J)
    assert tuple(o) == STAGE_OUTPUTS["score"]
    check(eng, "gpmp2mi_multi_plan_score", dict(inter_step=J), o, mp.h)
    kw = dict(inter_step=J, required_clearance=0.125, require_in_range=True)
    res = mp.select(**kw)
    assert list(res) == ["best", "n_eligible", "traj_best", "dense_best"]
    assert len(check(eng, "gpmp2mi_multi_plan_select", kw, res, mp.h)) == len(kw)
    eng.lib = FakeLib(write=False)
    res = mp.select(**kw)
    assert res == dict(best=-1, n_eligible=0, traj_best=None, dense_best=None)


def test_results_and_queues_of_plan_and_multi_plan(world):
    eng, pl = world
    mp = engine.MultiPlan(eng, Stub(0x100), Stub(0x200), pl.setting, B, [0, 0])
    keys = ["traj", "iters", "final_error", "status", "error_trace"]
    M = 3
    rows = dict(start_conf=np.zeros((M, D)), start_vel=np.ones((M, D)), end_conf=np.zeros((M, D)), end_vel=np.ones((M, D)))
    for p, prefix in ((pl, "gpmp2mi_plan_"), (mp, "gpmp2mi_multi_plan_")):
        res = p.result()
        assert list(res) == keys and res["traj"].shape == (B, N + 1, 2 * D)
        assert res["error_trace"].shape == (B, pl.setting.max_iter + 1) and res["iters"].dtype == np.int32
        check(eng, prefix + "get_result", {}, res, p.h)
        kw = dict(rows, init=np.zeros((M, N + 1, 2 * D)))
        res = p.optimize_queue(**kw)
        assert list(res) == keys and res["traj"].shape == (M, N + 1, 2 * D) and res["status"].shape == (M,)
        assert len(check(eng, prefix + "optimize_queue", kw, res, p.h)) == len(kw)
        assert eng.lib.calls[-1][1][1] == M
        kw = dict(rows, seed=7, first=2, scale=0.5, keep_first=True, mean=np.zeros((M, N + 1, 2 * D)))
        res = p.optimize_queue_seeded(want_init=True, **kw)
        assert list(res) == keys + ["init"]
        init = res.pop("init")
        assert len(check(eng, prefix + "optimize_queue_seeded", kw, res, p.h)) == len(kw)
        pars = [name for _, name in header_params(prefix + "optimize_queue_seeded")]
        assert init.shape == (M, N + 1, 2 * D) and init.flat[0] == pars.index("init_out")
        assert list(p.optimize_queue_seeded(**kw)) == keys and eng.lib.calls[-1][1][-1] is None


def test_the_checks_come_before_the_library(world):
    eng, pl = world
    eng.lib.calls.clear()
    with pytest.raises(ValueError, match="inter_step must be >= 0"):
        pl.select(-1)
    with pytest.raises(ValueError, match="required_pos_margin / max_time_scale must not be NaN"):
        pl.select_feasible(J, None, max_time_scale=float("nan"))
    with pytest.raises(ValueError, match="required_pos_margin / max_duration must not be NaN"):
        pl.select_retimed_dev(J, None, max_duration=float("nan"))
    with pytest.raises(ValueError, match="delta_t must be > 0"):
        eng.motion_score_traj(Stub(1), None, 0.0, J, np.zeros((B, N + 1, 2 * D)))
    with pytest.raises(ValueError, match=r"traj: expected \[B\]\[N\+1\]\[4\]"):
        eng.score_traj(Stub(1), Stub(2), 0.1, J, np.zeros((B, N + 1, 3)))
    with pytest.raises(ValueError, match=r"unknown path outputs: \['nope'\]"):
        pl.path_score(J, out=dict(nope=None))
    with pytest.raises(ValueError, match=r"unknown score outputs: \['nope'\]"):
        pl.moving_score(J, out=dict(nope=None))
    with pytest.raises(ValueError, match=r"tau: expected a contiguous float64 array of shape \[2, 5, 2\]"):
        pl.torque_score(Stub(3), J, out=dict(tau=np.zeros((2, 5, 3))))
    with pytest.raises(ValueError, match="these limits are for dof 3, not 2"):
        pl.retime(engine.MotionLimits(3), J)
    assert eng.lib.calls == []


def test_dev_tensors_are_checked_before_the_library_is_looked_at():
    """a plan without an engine: a mis-shaped tensor is refused before any attribute of the library is asked for"""
    class Tensor:
        dtype, shape, device = "torch.float64", (1, 1), type("d", (), {"type": "cuda"})()

        def is_contiguous(self):
            return True

        def data_ptr(self):
            raise AssertionError("a mis-shaped tensor was accepted")

    pl = engine.Plan.__new__(engine.Plan)
    pl.eng, pl.B, pl.N, pl.D = None, B, N, D
    for method, (_, kw, _, _) in selection_cases().items():
        with pytest.raises(ValueError, match="dense_best: expected a contiguous torch.float64 cuda tensor of shape"):
            getattr(pl, method + "_dev")(inter_step=J, dense_best=Tensor(), **kw)
    for key, outs in STAGE_OUTPUTS.items():
        name = [n for n in outs if n != "worst"][0]
        with pytest.raises(ValueError, match=name + ": expected a contiguous torch.float64 cuda tensor of shape"):
            getattr(pl, PLAN_METHOD[key] + "_dev")(inter_step=J, **{name: Tensor()}, **stage_inputs()[key])
