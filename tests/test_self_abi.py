"""The self-collision check (include/gpmp2mi.h "self-collision check") as far as it can be checked without a GPU: the
ABI is declared and exported, and argument errors are reported before any device work.  A pair table is bound to a robot
handle, and robot handles live on a device, so what needs a live handle -- the id checks of create, generate, an empty
table being accepted -- is in tests/test_gpu_self.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpmp2_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_NAMES = ["gpmp2mi_self_pairs_create", "gpmp2mi_self_pairs_generate", "gpmp2mi_self_pairs_count",
             "gpmp2mi_self_pairs_get", "gpmp2mi_self_score_traj", "gpmp2mi_self_score_traj_dev",
             "gpmp2mi_plan_self_score", "gpmp2mi_plan_self_score_dev", "gpmp2mi_plan_select_checked",
             "gpmp2mi_plan_select_checked_dev"]


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def test_entry_points_are_declared_and_exported(eng):
    hdr = open(os.path.join(ROOT, "include", "gpmp2mi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in INT_NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr), f"{n} is not declared in include/gpmp2mi.h"
        assert hasattr(eng.lib, n), f"{n} is not exported"
    assert re.search(r"\bvoid\s+gpmp2mi_self_pairs_destroy\s*\(", hdr) and hasattr(eng.lib, "gpmp2mi_self_pairs_destroy")
    assert re.search(r"typedef\s+struct\s+gpmp2mi_self_pairs\s+gpmp2mi_self_pairs\s*;", hdr)


def test_null_and_negative_arguments_are_refused_before_any_device_work(eng):
    lib = eng.lib
    t = np.zeros((1, 3, 4))
    data = np.array([[0.0, 1.0, 0.0, 1.0]])
    one = C.c_void_p(1)   # a non-null handle that must never be looked at: the null / negative argument is reported first
    out = C.c_void_p(7)
    best, n = C.c_int(7), C.c_int(7)
    calls = {
        "create robot": lambda: lib.gpmp2mi_self_pairs_create(None, 1, E.dptr(data), C.byref(out)),
        "create out": lambda: lib.gpmp2mi_self_pairs_create(one, 1, E.dptr(data), None),
        "create P": lambda: lib.gpmp2mi_self_pairs_create(one, -1, E.dptr(data), C.byref(out)),
        "create data": lambda: lib.gpmp2mi_self_pairs_create(one, 1, None, C.byref(out)),
        "generate robot": lambda: lib.gpmp2mi_self_pairs_generate(None, 2, 0, None, 0.0, 1.0, C.byref(out)),
        "generate out": lambda: lib.gpmp2mi_self_pairs_generate(one, 2, 0, None, 0.0, 1.0, None),
        "get table": lambda: lib.gpmp2mi_self_pairs_get(None, E.dptr(data)),
        "score_traj robot": lambda: lib.gpmp2mi_self_score_traj(None, one, 0.1, 0, 1, 2, E.dptr(t), None, None, None, None, None),
        "score_traj pairs": lambda: lib.gpmp2mi_self_score_traj(one, None, 0.1, 0, 1, 2, E.dptr(t), None, None, None, None, None),
        "score_traj traj": lambda: lib.gpmp2mi_self_score_traj(one, one, 0.1, 0, 1, 2, None, None, None, None, None, None),
        "score_traj_dev robot": lambda: lib.gpmp2mi_self_score_traj_dev(None, one, 0.1, 0, 1, 2, one, None, None, None, None, None, None),
        "score_traj_dev pairs": lambda: lib.gpmp2mi_self_score_traj_dev(one, None, 0.1, 0, 1, 2, one, None, None, None, None, None, None),
        "score_traj_dev traj": lambda: lib.gpmp2mi_self_score_traj_dev(one, one, 0.1, 0, 1, 2, None, None, None, None, None, None, None),
        "plan_self_score plan": lambda: lib.gpmp2mi_plan_self_score(None, one, 0, None, None, None, None, None),
        "plan_self_score pairs": lambda: lib.gpmp2mi_plan_self_score(one, None, 0, None, None, None, None, None),
        "plan_self_score_dev plan": lambda: lib.gpmp2mi_plan_self_score_dev(None, one, 0, None, None, None, None, None, None),
        "plan_self_score_dev pairs": lambda: lib.gpmp2mi_plan_self_score_dev(one, None, 0, None, None, None, None, None, None),
        "select_checked plan": lambda: lib.gpmp2mi_plan_select_checked(None, 0, 0.0, 0, one, 0.0, C.byref(best), C.byref(n), None, None),
        "select_checked pairs": lambda: lib.gpmp2mi_plan_select_checked(one, 0, 0.0, 0, None, 0.0, C.byref(best), C.byref(n), None, None),
        "select_checked_dev plan": lambda: lib.gpmp2mi_plan_select_checked_dev(None, 0, 0.0, 0, one, 0.0, None, None, None, None, None),
        "select_checked_dev pairs": lambda: lib.gpmp2mi_plan_select_checked_dev(one, 0, 0.0, 0, None, 0.0, None, None, None, None, None),
    }
    for name, call in calls.items():
        assert call() == 1, name
        assert len(lib.gpmp2mi_last_error()) > 0, name
    assert (best.value, n.value) == (7, 7)      # a refused call writes nothing
    assert lib.gpmp2mi_self_pairs_count(None) == -1
    lib.gpmp2mi_self_pairs_destroy(None)        # a no-op


def test_python_wrappers_refuse_bad_input_before_the_library_is_called():
    class Boom:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name})")

    class Handle:
        ptr, dof, S = None, 7, 16

    eng = E.Engine.__new__(E.Engine)
    eng.lib = Boom()
    r, t = Handle(), Handle()
    for bad in ([[0, 16, 0, 1]], [[3, 3, 0, 1]], [[0.5, 1, 0, 1]], [[-1, 2, 0, 1]], np.zeros((2, 5))):
        with pytest.raises(ValueError):
            eng.self_pairs(r, bad)
    with pytest.raises(ValueError):
        eng.generate_self_pairs(r, min_joint_gap=0)
    with pytest.raises(ValueError):
        eng.generate_self_pairs(r, ref_conf=np.zeros((2, 6)))
    good = np.zeros((2, 5, 14))
    for bad in (np.zeros((2, 5, 13)), np.zeros((2, 5)), np.zeros((2, 1, 14))):
        with pytest.raises(ValueError):
            eng.self_score_traj(r, t, 0.1, 2, bad)
    with pytest.raises(ValueError):
        eng.self_score_traj(r, t, 0.1, -1, good)
    with pytest.raises(ValueError):
        eng.self_score_traj(r, t, 0.0, 1, good)
    for out in ({"self_dense_cost": np.zeros(3)}, {"worst": np.zeros((2, 2))}, {"invalid": np.zeros(2)},
                {"dense_cost": np.zeros(2)}):
        with pytest.raises(ValueError):
            eng.self_score_traj(r, t, 0.1, 1, good, out=out)
    pl = E.Plan.__new__(E.Plan)
    pl.eng, pl.B, pl.N, pl.D = eng, 2, 4, 7
    with pytest.raises(ValueError):
        pl.self_score(t, 1, out={"self_dense_cost": np.zeros(5)})
    with pytest.raises(ValueError):
        pl.self_score(t, -1)
    with pytest.raises(ValueError):
        pl.select_checked(-2, t)
    with pytest.raises(ValueError):
        pl.select_checked_dev(-2, t)
