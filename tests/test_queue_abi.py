"""CPU-side checks of the queue entry points (no GPU needed): they are declared in include/gpmp2mi.h (and so covered
by the export test), refuse a NULL plan, and the Python wrapper refuses inputs that disagree on the number of
problems before anything reaches the library."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUEUE = ["gpmp2mi_plan_optimize_queue", "gpmp2mi_plan_optimize_queue_dev", "gpmp2mi_plan_queue_stats"]


def test_queue_entry_points_are_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpmp2mi.h")).read(), flags=re.S)
    for name in QUEUE:
        assert re.search(rf"\b{name}\s*\(", text), name
    lib = ctypes.CDLL(os.path.join(ROOT, "gpmp2_amd", "csrc", "libgpmp2mi.so"))
    for name in QUEUE:
        assert hasattr(lib, name), name


def test_null_plan_is_invalid():
    from gpmp2_amd import _capi, engine
    lib = engine.load_library()
    z = np.zeros(7)
    args = [engine.dptr(z)] * 5
    assert lib.gpmp2mi_plan_optimize_queue(None, 1, *args, None, None, None, None, None) == 1
    assert b"null plan" in lib.gpmp2mi_last_error()
    assert lib.gpmp2mi_plan_optimize_queue_dev(None, 1, *[1] * 5, None, None, None, None, None, None) == 1
    st = _capi.QueueStats()
    assert lib.gpmp2mi_plan_queue_stats(None, ctypes.byref(st)) == 1


def test_wrapper_rejects_disagreeing_rows():
    from gpmp2_amd import engine
    D, N = 3, 4
    ok = [np.zeros((5, D))] * 4 + [np.zeros((5, N + 1, 2 * D))]
    M, rows, t = engine.queue_inputs(D, N, *ok)
    assert M == 5 and t.shape == (5, N + 1, 2 * D)
    with pytest.raises(ValueError, match="disagree"):
        engine.queue_inputs(D, N, np.zeros((5, D)), np.zeros((4, D)), np.zeros((5, D)), np.zeros((5, D)),
                            np.zeros((5, N + 1, 2 * D)))
    with pytest.raises(ValueError, match="disagree"):
        engine.queue_inputs(D, N, *ok[:4], np.zeros((6, N + 1, 2 * D)))
    with pytest.raises(ValueError, match="init"):
        engine.queue_inputs(D, N, *ok[:4], np.zeros((5, N, 2 * D)))
    with pytest.raises(ValueError, match="start_conf"):
        engine.queue_inputs(D, N, np.zeros((5, D + 1)), *ok[1:])
