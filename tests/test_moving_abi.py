"""Moving obstacles (include/gpmp2mi.h "moving obstacles") as far as they can be checked without a GPU: the ABI is
declared and exported, argument errors are reported before any device work, gpmp2mi_graph_opts grew at its end only and
its ctypes mirror has the header's size.  What needs a live plan -- the capacity, the poisoned plan, a plan without
room -- is in tests/test_gpu_moving.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gpmp2_amd import _capi
from gpmp2_amd import engine as E
from gpmp2_amd.settings import TrajOptimizerSetting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_NAMES = ["gpmp2mi_plan_set_moving_spheres", "gpmp2mi_plan_set_moving_spheres_dev", "gpmp2mi_moving_sphere_factor",
             "gpmp2mi_moving_score_traj", "gpmp2mi_moving_score_traj_dev", "gpmp2mi_plan_moving_score",
             "gpmp2mi_plan_moving_score_dev", "gpmp2mi_plan_select_moving", "gpmp2mi_plan_select_moving_dev"]
NEW_FIELDS = ["max_moving_spheres", "moving_first", "moving_last", "moving_epsilon", "moving_sigma"]


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def test_entry_points_are_declared_and_exported(eng):
    hdr = open(os.path.join(ROOT, "include", "gpmp2mi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in INT_NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr), f"{n} is not declared in include/gpmp2mi.h"
        assert hasattr(eng.lib, n), f"{n} is not exported"
    assert re.search(r"#define\s+GPMP2MI_MAX_MOVING_SPHERES\s+64\b", hdr)
    assert _capi.MAX_MOVING_SPHERES == 64


def test_null_negative_and_oversized_arguments_are_refused_before_any_device_work(eng):
    lib = eng.lib
    t = np.zeros((1, 3, 4))
    rad, cen = np.full(65, 0.1), np.zeros((65, 3, 3))
    conf, err = np.zeros((1, 2)), np.zeros(8)
    one = C.c_void_p(1)   # a non-null handle that must never be looked at: the bad argument is reported first
    best, n = C.c_int(7), C.c_int(7)
    r_, c_, t_ = E.dptr(rad), E.dptr(cen), E.dptr(t)
    none5 = (None,) * 5
    calls = {
        "set plan": lambda: lib.gpmp2mi_plan_set_moving_spheres(None, 1, r_, c_),
        "set K < 0": lambda: lib.gpmp2mi_plan_set_moving_spheres(one, -1, r_, c_),
        "set K > max": lambda: lib.gpmp2mi_plan_set_moving_spheres(one, 65, r_, c_),
        "set radius": lambda: lib.gpmp2mi_plan_set_moving_spheres(one, 1, None, c_),
        "set centers": lambda: lib.gpmp2mi_plan_set_moving_spheres(one, 1, r_, None),
        "set_dev plan": lambda: lib.gpmp2mi_plan_set_moving_spheres_dev(None, 1, one, one, None),
        "set_dev K < 0": lambda: lib.gpmp2mi_plan_set_moving_spheres_dev(one, -1, one, one, None),
        "set_dev K > max": lambda: lib.gpmp2mi_plan_set_moving_spheres_dev(one, 65, one, one, None),
        "set_dev radius": lambda: lib.gpmp2mi_plan_set_moving_spheres_dev(one, 1, None, one, None),
        "set_dev centers": lambda: lib.gpmp2mi_plan_set_moving_spheres_dev(one, 1, one, None, None),
        "factor robot": lambda: lib.gpmp2mi_moving_sphere_factor(None, 1, r_, 0.1, 1, E.dptr(conf), c_, E.dptr(err), None),
        "factor conf": lambda: lib.gpmp2mi_moving_sphere_factor(one, 1, r_, 0.1, 1, None, c_, E.dptr(err), None),
        "factor err": lambda: lib.gpmp2mi_moving_sphere_factor(one, 1, r_, 0.1, 1, E.dptr(conf), c_, None, None),
        "factor M < 0": lambda: lib.gpmp2mi_moving_sphere_factor(one, 1, r_, 0.1, -1, E.dptr(conf), c_, E.dptr(err), None),
        "factor K < 0": lambda: lib.gpmp2mi_moving_sphere_factor(one, -1, r_, 0.1, 1, E.dptr(conf), c_, E.dptr(err), None),
        "factor K > max": lambda: lib.gpmp2mi_moving_sphere_factor(one, 65, r_, 0.1, 1, E.dptr(conf), c_, E.dptr(err), None),
        "factor radius": lambda: lib.gpmp2mi_moving_sphere_factor(one, 1, None, 0.1, 1, E.dptr(conf), c_, E.dptr(err), None),
        "factor centers": lambda: lib.gpmp2mi_moving_sphere_factor(one, 1, r_, 0.1, 1, E.dptr(conf), None, E.dptr(err), None),
        "factor epsilon": lambda: lib.gpmp2mi_moving_sphere_factor(one, 1, r_, np.nan, 1, E.dptr(conf), c_, E.dptr(err), None),
        "score_traj robot": lambda: lib.gpmp2mi_moving_score_traj(None, 1, r_, c_, 0.1, 0.1, 0, 1, 2, t_, *none5),
        "score_traj traj": lambda: lib.gpmp2mi_moving_score_traj(one, 1, r_, c_, 0.1, 0.1, 0, 1, 2, None, *none5),
        "score_traj K < 0": lambda: lib.gpmp2mi_moving_score_traj(one, -1, r_, c_, 0.1, 0.1, 0, 1, 2, t_, *none5),
        "score_traj K > max": lambda: lib.gpmp2mi_moving_score_traj(one, 65, r_, c_, 0.1, 0.1, 0, 1, 2, t_, *none5),
        "score_traj radius": lambda: lib.gpmp2mi_moving_score_traj(one, 1, None, c_, 0.1, 0.1, 0, 1, 2, t_, *none5),
        "score_traj centers": lambda: lib.gpmp2mi_moving_score_traj(one, 1, r_, None, 0.1, 0.1, 0, 1, 2, t_, *none5),
        "score_traj epsilon": lambda: lib.gpmp2mi_moving_score_traj(one, 1, r_, c_, np.nan, 0.1, 0, 1, 2, t_, *none5),
        "score_traj inter": lambda: lib.gpmp2mi_moving_score_traj(one, 1, r_, c_, 0.1, 0.1, -1, 1, 2, t_, *none5),
        "score_traj B": lambda: lib.gpmp2mi_moving_score_traj(one, 1, r_, c_, 0.1, 0.1, 0, -1, 2, t_, *none5),
        "score_traj N": lambda: lib.gpmp2mi_moving_score_traj(one, 1, r_, c_, 0.1, 0.1, 0, 1, 0, t_, *none5),
        "score_traj dt": lambda: lib.gpmp2mi_moving_score_traj(one, 1, r_, c_, 0.1, 0.0, 0, 1, 2, t_, *none5),
        "score_traj_dev robot": lambda: lib.gpmp2mi_moving_score_traj_dev(None, 1, one, one, 0.1, 0.1, 0, 1, 2, one, *none5, None),
        "score_traj_dev traj": lambda: lib.gpmp2mi_moving_score_traj_dev(one, 1, one, one, 0.1, 0.1, 0, 1, 2, None, *none5, None),
        "score_traj_dev K < 0": lambda: lib.gpmp2mi_moving_score_traj_dev(one, -1, one, one, 0.1, 0.1, 0, 1, 2, one, *none5, None),
        "score_traj_dev K > max": lambda: lib.gpmp2mi_moving_score_traj_dev(one, 65, one, one, 0.1, 0.1, 0, 1, 2, one, *none5, None),
        "score_traj_dev radius": lambda: lib.gpmp2mi_moving_score_traj_dev(one, 1, None, one, 0.1, 0.1, 0, 1, 2, one, *none5, None),
        "plan_moving_score plan": lambda: lib.gpmp2mi_plan_moving_score(None, 0, *none5),
        "plan_moving_score_dev plan": lambda: lib.gpmp2mi_plan_moving_score_dev(None, 0, *none5, None),
        "select_moving plan": lambda: lib.gpmp2mi_plan_select_moving(None, 0, 0.0, 0, None, 0.0, 0.0, C.byref(best), C.byref(n), None, None),
        "select_moving_dev plan": lambda: lib.gpmp2mi_plan_select_moving_dev(None, 0, 0.0, 0, None, 0.0, 0.0, None, None, None, None, None),
    }
    for name, call in calls.items():
        assert call() == 1, name
        assert len(lib.gpmp2mi_last_error()) > 0, name
    assert (best.value, n.value) == (7, 7)      # a refused call writes nothing


def test_graph_opts_default_leaves_the_new_fields_zero(eng):
    o = _capi.GraphOpts()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    eng.lib.gpmp2mi_graph_opts_default(C.byref(o))
    assert (o.max_moving_spheres, o.moving_first, o.moving_last) == (0, 0, 0)
    assert (o.moving_epsilon, o.moving_sigma) == (0.0, 0.0)
    assert o.lm_lambda_initial == 100.0 and o.n_self_collision == 0
    # the new fields are the struct's last ones, in the header's order
    assert [name for name, _ in _capi.GraphOpts._fields_][-5:] == NEW_FIELDS


def test_graph_opts_mirror_has_the_size_and_offsets_of_the_header(tmp_path):
    src = tmp_path / "opts_size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gpmp2mi.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(gpmp2mi_graph_opts));\n'
                   + "".join(f'  printf(" %zu", offsetof(gpmp2mi_graph_opts, {f}));\n' for f in NEW_FIELDS)
                   + '  printf(" %zu\\n", offsetof(gpmp2mi_graph_opts, self_collision));\n  return 0;\n}\n')
    exe = tmp_path / "opts_size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(_capi.GraphOpts)] + [getattr(_capi.GraphOpts, f).offset for f in NEW_FIELDS + ["self_collision"]]
    assert got == want, (got, want)


def test_settings_carry_the_capacity_and_the_constants():
    s = TrajOptimizerSetting(7)
    s.set_total_step(12)
    _, o, _ = _capi.make_settings(s)
    assert (o.max_moving_spheres, o.moving_first, o.moving_last, o.moving_epsilon, o.moving_sigma) == (0, 0, 0, 0.0, 0.0)
    s.set_moving_spheres(8, 0.2, 0.01)
    _, o, _ = _capi.make_settings(s)
    assert (o.max_moving_spheres, o.moving_first, o.moving_last, o.moving_epsilon, o.moving_sigma) == (8, 0, 12, 0.2, 0.01)
    s.set_moving_spheres(3, 0.1, 0.5, states=(1, 11))
    _, o, _ = _capi.make_settings(s)
    assert (o.max_moving_spheres, o.moving_first, o.moving_last) == (3, 1, 11)
    s.set_moving_spheres(65, 0.1, 0.5)
    with pytest.raises(ValueError):
        _capi.make_settings(s)


def test_python_wrappers_refuse_bad_input_before_the_library_is_called():
    class Boom:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name})")

    class Handle:
        ptr, dof, S = None, 7, 16

    eng = E.Engine.__new__(E.Engine)
    eng.lib = Boom()
    r = Handle()
    good = np.zeros((2, 5, 14))
    rad, cen = np.full(2, 0.1), np.zeros((2, 5, 3))
    for bad in (np.zeros((2, 4, 3)), np.zeros((3, 5, 3)), np.zeros((2, 5))):
        with pytest.raises(ValueError):
            eng.moving_score_traj(r, rad, bad, 0.1, 0.1, 1, good)
    with pytest.raises(ValueError):
        eng.moving_score_traj(r, np.full(65, 0.1), np.zeros((65, 5, 3)), 0.1, 0.1, 1, good)
    with pytest.raises(ValueError):
        eng.moving_score_traj(r, rad, cen, 0.1, 0.1, -1, good)
    with pytest.raises(ValueError):
        eng.moving_score_traj(r, rad, cen, 0.1, 0.0, 1, good)
    for out in ({"worst": np.zeros((2, 2), dtype=np.int32)}, {"dense_cost": np.zeros(2)}, {"invalid": np.zeros(2)}):
        with pytest.raises(ValueError):
            eng.moving_score_traj(r, rad, cen, 0.1, 0.1, 1, good, out=out)
    with pytest.raises(ValueError):
        eng.moving_sphere_factor(r, np.full(65, 0.1), 0.1, np.zeros((1, 7)), np.zeros((1, 65, 3)))
    pl = E.Plan.__new__(E.Plan)
    pl.eng, pl.B, pl.N, pl.D = eng, 2, 4, 7
    with pytest.raises(ValueError):
        pl.set_moving_spheres(rad, np.zeros((2, 4, 3)))
    with pytest.raises(ValueError):
        pl.moving_score(-1)
    with pytest.raises(ValueError):
        pl.moving_score(1, out={"moving_dense_cost": np.zeros(5)})
    with pytest.raises(ValueError):
        pl.select_moving(-2)
    with pytest.raises(ValueError):
        pl.select_moving_dev(-2)
