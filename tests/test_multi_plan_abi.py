"""CPU-side checks of the multi-device plan entry points (no GPU needed): they are declared in include/gpmp2mi.h /
gpmp2mi_debug.h and exported, every entry point refuses a NULL multi plan with a message, create refuses NULL and
out-of-range arguments before it looks for a device, and the Python wrapper refuses bad inputs before anything reaches
the library."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = ["gpmp2mi_multi_plan_create", "gpmp2mi_multi_plan_destroy", "gpmp2mi_multi_plan_shards",
          "gpmp2mi_multi_plan_set_problem", "gpmp2mi_multi_plan_optimize", "gpmp2mi_multi_plan_get_result",
          "gpmp2mi_multi_plan_get_result_dev", "gpmp2mi_multi_plan_optimize_queue", "gpmp2mi_multi_plan_queue_stats"]
DEBUG = ["gpmp2mi_debug_multi_plan_create", "gpmp2mi_debug_replica_counts", "gpmp2mi_debug_current_device"]


def _decl(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


def test_multi_plan_entry_points_are_declared_and_exported():
    pub, dbg = _decl("gpmp2mi.h"), _decl("gpmp2mi_debug.h")
    for name in PUBLIC:
        assert re.search(rf"\b{name}\s*\(", pub), name
    for name in DEBUG:
        assert re.search(rf"\b{name}\s*\(", dbg), name
    assert re.search(r"#define GPMP2MI_MAX_SHARDS 16\b", pub)
    lib = ctypes.CDLL(os.path.join(ROOT, "gpmp2_amd", "csrc", "libgpmp2mi.so"))
    for name in PUBLIC + DEBUG:
        assert hasattr(lib, name), name


def test_null_multi_plan_is_invalid_everywhere():
    from gpmp2_amd import _capi, engine
    lib = engine.load_library()
    z = np.zeros(64)
    d = engine.dptr(z)
    it = np.zeros(8, dtype=np.int32)
    i = engine.iptr(it)
    calls = {
        "shards": lambda: lib.gpmp2mi_multi_plan_shards(None, i, i, i),
        "set_problem": lambda: lib.gpmp2mi_multi_plan_set_problem(None, d, d, d, d, d),
        "optimize": lambda: lib.gpmp2mi_multi_plan_optimize(None),
        "get_result": lambda: lib.gpmp2mi_multi_plan_get_result(None, d, i, d, i, d),
        "get_result_dev": lambda: lib.gpmp2mi_multi_plan_get_result_dev(None, 0, None, None, None, None, None),
        "optimize_queue": lambda: lib.gpmp2mi_multi_plan_optimize_queue(None, 1, d, d, d, d, d, d, i, d, i, d),
        "queue_stats": lambda: lib.gpmp2mi_multi_plan_queue_stats(None, 0, ctypes.byref(_capi.QueueStats())),
    }
    for name, call in calls.items():
        lib.gpmp2mi_last_error  # reset nothing: every call must set its own message
        assert call() == 1, name
        assert b"null multi plan" in lib.gpmp2mi_last_error(), name
    lib.gpmp2mi_multi_plan_destroy(None)   # a no-op
    r, s = ctypes.c_long(-1), ctypes.c_long(-1)
    assert lib.gpmp2mi_debug_replica_counts(ctypes.byref(r), ctypes.byref(s)) == 0 and r.value >= 0 and s.value >= 0
    assert lib.gpmp2mi_debug_replica_counts(None, None) == 0


def test_create_refuses_bad_arguments_before_looking_for_a_device():
    """NULL arguments, nshards outside 1..16 and B < nshards are GPMP2MI_ERR_INVALID whether or not a GPU is present
    (dummy non-NULL handles: nothing is dereferenced before these checks)"""
    from gpmp2_amd import engine
    lib = engine.load_library()
    out = ctypes.c_void_p()
    fake = ctypes.c_void_p(8)   # never dereferenced: the argument checks come first
    devs = np.zeros(17, dtype=np.int32)
    dv = engine.iptr(devs)
    create = lib.gpmp2mi_multi_plan_create
    assert create(None, fake, fake, None, 4, 2, dv, ctypes.byref(out)) == 1
    assert b"null argument" in lib.gpmp2mi_last_error()
    assert create(fake, None, fake, None, 4, 2, dv, ctypes.byref(out)) == 1
    assert create(fake, fake, None, None, 4, 2, dv, ctypes.byref(out)) == 1
    assert create(fake, fake, fake, None, 4, 2, None, ctypes.byref(out)) == 1
    assert create(fake, fake, fake, None, 4, 2, dv, None) == 1
    assert create(fake, fake, fake, None, 4, 0, dv, ctypes.byref(out)) == 1
    assert b"nshards" in lib.gpmp2mi_last_error()
    assert create(fake, fake, fake, None, 64, 17, dv, ctypes.byref(out)) == 1
    assert create(fake, fake, fake, None, 3, 4, dv, ctypes.byref(out)) == 1
    assert b"nshards" in lib.gpmp2mi_last_error() and out.value is None
    assert lib.gpmp2mi_debug_multi_plan_create(fake, fake, fake, None, 1, 2, dv, None, 1, ctypes.byref(out)) == 1


def test_create_without_a_gpu_is_no_device():
    from gpmp2_amd import engine
    eng = engine.Engine()
    if eng.device_count() > 0:
        pytest.skip("a GPU is present; the no-device answer is only observable without one")
    lib = eng.lib
    out = ctypes.c_void_p()
    fake = ctypes.c_void_p(8)
    dv = engine.iptr(np.zeros(2, dtype=np.int32))
    assert lib.gpmp2mi_multi_plan_create(fake, fake, fake, None, 4, 2, dv, ctypes.byref(out)) == 2


def test_wrapper_rejects_bad_inputs_before_the_library():
    from gpmp2_amd import engine

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError(f"reached the library: {name}")

    class Eng:
        lib = NoLib()

    class Setting:
        dof, total_step, max_iter = 3, 4, 10

    with pytest.raises(ValueError, match="at least one device"):
        engine.MultiPlan(Eng(), None, None, Setting(), 4, [])
    with pytest.raises(ValueError, match="smaller than the number of shards"):
        engine.MultiPlan(Eng(), None, None, Setting(), 2, [0, 0, 0])
    with pytest.raises(ValueError, match="at most 16"):
        engine.MultiPlan(Eng(), None, None, Setting(), 64, [0] * 17)
    assert engine.multi_plan_args(5, (0, 1)) == (5, [0, 1])
    # row-count checks of set_problem / optimize_queue (queue_inputs) run before any library call
    mp = engine.MultiPlan.__new__(engine.MultiPlan)
    mp.eng, mp.D, mp.N, mp.T, mp.B, mp.h = Eng(), 3, 4, 11, 5, None
    ok = [np.zeros((5, 3))] * 4 + [np.zeros((5, 5, 6))]
    with pytest.raises(ValueError, match="disagree"):
        mp.set_problem(np.zeros((5, 3)), np.zeros((4, 3)), *ok[2:])
    with pytest.raises(ValueError, match="expected 5 rows"):
        mp.set_problem(*[x[:4] for x in ok])
    with pytest.raises(ValueError, match="disagree"):
        mp.optimize_queue(*ok[:4], np.zeros((6, 5, 6)))
    with pytest.raises(ValueError, match="init"):
        mp.optimize_queue(*ok[:4], np.zeros((5, 4, 6)))
