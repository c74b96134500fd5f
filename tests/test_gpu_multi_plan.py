"""One batch sharded over several devices of this process (gpmp2mi_multi_plan): every row returns exactly what one plan
returns for it -- value-identical trajectories, final errors and error traces, identical iteration counts and status
codes -- whether the shards share a device, run on copies of the robot and the field, or run on another GPU."""
import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from gpmp2_amd import engine as E
from gpmp2_amd import problems
from test_gpu_plan_queue import _assert_same, _expand, _rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _handles(engine, p):
    return engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)


def _one_plan(engine, r, s, p, forms=None):
    pl = engine.plan(r, s, p.setting, p.B, forms)
    pl.set_problem(*_rows(p))
    pl.optimize()
    res = pl.result()
    pl.close()
    return res


def _multi(engine, r, s, p, devices, **kw):
    mp = engine.multi_plan(r, s, p.setting, p.B, devices, **kw)
    mp.set_problem(*_rows(p))
    mp.optimize()
    return mp, mp.result()


def _wam_small(opt, B):
    return problems.wam_restarts(B=B, total_step=12, obs_check_inter=3, opt=opt, sdf="40")


def _counts(engine):
    v = [ctypes.c_long() for _ in range(5)]
    assert engine.lib.gpmp2mi_debug_resource_counts(*[ctypes.byref(x) for x in v]) == 0
    return dict(live_chunks=v[0].value, live_flagbufs=v[2].value)


def _device(engine, set_to=-1):
    """the calling thread's current device in the library's HIP runtime (after making set_to current, if >= 0)"""
    d = ctypes.c_int(-1)
    engine._ck(engine.lib.gpmp2mi_debug_current_device(int(set_to), ctypes.byref(d)))
    return d.value


def test_headline_wam_two_shards_of_device_0(engine):
    p = problems.wam_restarts(B=64, opt="GN")
    r, s = _handles(engine, p)
    mp, res = _multi(engine, r, s, p, [0, 0])
    assert mp.shards() == ([0, 0], [0, 32, 64])
    assert len(set(res["iters"])) > 1
    _assert_same(res, _one_plan(engine, r, s, p))
    mp.close()


@pytest.mark.parametrize("opt", ["GN", "LM", "DOGLEG"])
def test_uneven_three_shards_every_optimizer(engine, opt):
    p = _wam_small(opt, 10)
    r, s = _handles(engine, p)
    mp, res = _multi(engine, r, s, p, [0, 0, 0])
    assert mp.shards() == ([0, 0, 0], [0, 4, 7, 10])
    _assert_same(res, _one_plan(engine, r, s, p))
    mp.close()


def _point_robot(B):
    p = problems.point_robot_2d()
    p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init = _expand(p, B, 0.5)
    return p


def _mobile_arm(B):
    p = problems.mobile_arm_config5()
    p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init = _expand(p, B, 0.05)
    return p


@pytest.mark.parametrize("which", ["wam_3d", "point_2d", "mobile_arm_pose2"])
def test_replicas_on_the_same_device(engine, which):
    p = {"wam_3d": lambda: _wam_small("GN", 6), "point_2d": lambda: _point_robot(6),
         "mobile_arm_pose2": lambda: _mobile_arm(6)}[which]()
    r, s = _handles(engine, p)
    ref = _one_plan(engine, r, s, p)
    before, reps0 = _counts(engine), engine.replica_counts()
    mp, res = _multi(engine, r, s, p, [0, 0], replicate_all=True)
    assert engine.replica_counts() == (reps0[0] + 1, reps0[1] + 1)   # one copy of each, shared by both shards
    _assert_same(res, ref)
    mp.close()
    assert engine.replica_counts() == reps0
    assert _counts(engine) == before


def test_forced_form_reaches_every_shard(engine):
    p = _wam_small("GN", 8)
    r, s = _handles(engine, p)
    mp, res = _multi(engine, r, s, p, [0, 0], forms={"lin_split": 2})
    _assert_same(res, _one_plan(engine, r, s, p, forms={"lin_split": 2}))
    mp.close()


def test_queue_over_two_shards(engine):
    p = _wam_small("GN", 96)
    r, s = _handles(engine, p)
    ref = _one_plan(engine, r, s, p)
    mp = engine.multi_plan(r, s, p.setting, 16, [0, 0])
    q = mp.optimize_queue(*_rows(p))
    _assert_same(q, ref)
    for k in range(2):
        st = mp.queue_stats(k)
        assert 0 < st["busy_slot_passes"] <= st["slot_passes"] == 8 * st["passes"], st
    # a queue run leaves no problem behind
    with pytest.raises(E.Gpmp2miError) as ei:
        mp.result()
    assert ei.value.code == 1
    one = mp.optimize_queue(*[a[:1] for a in _rows(p)])
    _assert_same(one, {k: v[:1] for k, v in ref.items()})
    assert mp.queue_stats(0)["passes"] > 0
    assert mp.queue_stats(1) == dict(passes=0, slot_passes=0, busy_slot_passes=0)
    mp.close()


_GATHER = r"""
import numpy as np
import torch                      # torch's HIP runtime first, as bench.py does
torch.cuda.init()
from gpmp2_amd import engine as E, problems
eng = E.Engine()
p = problems.wam_restarts(B=10, total_step=12, obs_check_inter=3, opt="LM", sdf="40")
r, s = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
mp = eng.multi_plan(r, s, p.setting, p.B, [0, 0])
mp.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
mp.optimize()
res = mp.result()
B, N, D = p.B, p.setting.total_step, p.setting.dof
dev = torch.device("cuda:0")
traj = torch.full((B, N + 1, 2 * D), float("nan"), dtype=torch.float64, device=dev)
iters = torch.full((B,), -1, dtype=torch.int32, device=dev)
ferr = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
status = torch.full((B,), -1, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
st = torch.cuda.Stream(device=dev)
mp.result_dev(0, traj=traj, iters=iters, final_error=ferr, status=status, stream=st.cuda_stream)
with torch.cuda.stream(st):
    got = [t.cpu().numpy() for t in (traj, iters, ferr, status)]
assert np.array_equal(got[0], res["traj"]) and list(got[1]) == list(res["iters"])
assert np.array_equal(got[2], res["final_error"]) and list(got[3]) == list(res["status"])
try:
    mp.result_dev(0, traj=traj[:1], stream=st.cuda_stream)
    raise SystemExit("a wrong-shape tensor was accepted")
except ValueError:
    pass
mp.close()
print("GATHER OK")
"""


def test_gather_onto_a_device_on_a_torch_stream():
    """result_dev into torch tensors on a torch stream equals result(); in a fresh process that starts torch's HIP
    runtime before the library, as bench.py does"""
    if importlib.util.find_spec("torch") is None:   # not imported here: this process keeps the library's HIP runtime
        pytest.skip("torch is not installed")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + [x for x in [os.environ.get("PYTHONPATH")] if x]))
    r = subprocess.run([sys.executable, "-c", _GATHER], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0 and "GATHER OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_errors_and_the_current_device(engine):
    p = _wam_small("GN", 6)
    r, s = _handles(engine, p)
    lib, n = engine.lib, engine.device_count()
    here = n - 1
    _device(engine, here)
    try:
        with pytest.raises(E.Gpmp2miError) as ei:
            engine.multi_plan(r, s, p.setting, p.B, [0, n])
        assert ei.value.code == 1 and "out of range" in str(ei.value)
        assert _device(engine) == here
        sset, o, _ = E._capi.make_settings(p.setting)
        out = ctypes.c_void_p()
        devs = np.zeros(4, dtype=np.int32)
        assert lib.gpmp2mi_multi_plan_create(r.ptr, s.ptr, ctypes.byref(sset), ctypes.byref(o), 3, 4, E.iptr(devs),
                                             ctypes.byref(out)) == 1
        assert out.value is None
        mp = engine.multi_plan(r, s, p.setting, p.B, [0, 0])
        assert _device(engine) == here
        with pytest.raises(E.Gpmp2miError) as ei:
            mp.result()
        assert ei.value.code == 1 and "not been optimized" in str(ei.value)
        with pytest.raises(E.Gpmp2miError) as ei:
            mp.optimize()
        assert ei.value.code == 1
        with pytest.raises(E.Gpmp2miError) as ei:
            mp.queue_stats(0)
        assert ei.value.code == 1
        with pytest.raises(E.Gpmp2miError):
            mp.queue_stats(2)
        z = E.dptr(np.zeros(8))
        assert lib.gpmp2mi_multi_plan_optimize_queue(mp.h.ptr, 1, z, None, z, z, z, None, None, None, None, None) == 1
        assert lib.gpmp2mi_multi_plan_get_result_dev(mp.h.ptr, n, None, None, None, None, None) == 1
        mp.set_problem(*_rows(p))
        mp.optimize()
        assert _device(engine) == here
        _assert_same(mp.result(), _one_plan(engine, r, s, p))
        q = mp.optimize_queue(*_rows(p))
        assert _device(engine) == here
        _assert_same(q, mp.optimize_queue(*_rows(p)))
        mp.close()
        assert _device(engine) == here
    finally:
        _device(engine, 0)


def test_two_gpus(engine):
    if engine.device_count() < 2:
        pytest.skip("needs two GPUs")
    p = problems.wam_restarts(B=64, opt="GN")
    r, s = _handles(engine, p)
    reps0 = engine.replica_counts()
    mp, res = _multi(engine, r, s, p, [0, 1])
    assert mp.shards() == ([0, 1], [0, 32, 64])
    assert engine.replica_counts() == (reps0[0] + 1, reps0[1] + 1)
    _assert_same(res, _one_plan(engine, r, s, p))
    mp.close()
    assert engine.replica_counts() == reps0
