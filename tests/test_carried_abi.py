"""Carried object (include/gpmp2mi.h "carried object") as far as it can be checked without a GPU: the ABI is declared and
exported with the stated argument types, argument errors are reported before any device work, gpmp2mi_graph_opts grew
between self_collision and workspace_path only and its ctypes mirror has the header's size and offsets.  What needs a
live plan -- the capacity, a plan without room, the resident set after a refused call -- is in
tests/test_gpu_carried.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gpmp2_amd import _capi, scoring
from gpmp2_amd import engine as E
from gpmp2_amd.settings import TrajOptimizerSetting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, i, d, ip, f = C.c_void_p, C.c_int, _capi.c_double_p, _capi.c_int_p, C.c_double
ARGTYPES = {
    "gpmp2mi_plan_set_carried": [vp, i, i, d, d],
    "gpmp2mi_plan_set_carried_dev": [vp, i, i, vp, vp, vp],
    "gpmp2mi_plan_carried_count": [vp],
    "gpmp2mi_carried_sphere_factor": [vp, vp, i, i, d, d, f, i, d, d, d],
    "gpmp2mi_carried_score_traj": [vp, vp, i, i, d, d, f, i, i, i, d, d, d, d, ip, ip],
    "gpmp2mi_carried_score_traj_dev": [vp, vp, i, i, vp, vp, f, i, i, i] + [vp] * 7,
    "gpmp2mi_plan_carried_score": [vp, i, d, d, d, ip, ip],
    "gpmp2mi_plan_carried_score_dev": [vp, i] + [vp] * 6,
    "gpmp2mi_plan_select_carried": [vp, i, f, i, vp, f, f, ip, ip, d, d],
    "gpmp2mi_plan_select_carried_dev": [vp, i, f, i, vp, f, f] + [vp] * 5,
}
NEW_FIELDS = ["max_carried_spheres", "carried_first", "carried_last", "carried_epsilon", "carried_sigma"]


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def _header():
    hdr = open(os.path.join(ROOT, "include", "gpmp2mi.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_entry_points_are_declared_exported_and_typed(eng):
    hdr = _header()
    for n, args in ARGTYPES.items():
        m = re.search(r"\bint\s+" + n + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{n} is not declared in include/gpmp2mi.h"
        assert hasattr(eng.lib, n), f"{n} is not exported"
        fn = getattr(eng.lib, n)
        assert list(fn.argtypes) == args and fn.restype is C.c_int, n
        assert len(m.group(1).split(",")) == len(args), n            # as many parameters as the header declares
    assert re.search(r"#define\s+GPMP2MI_MAX_CARRIED_SPHERES\s+256\b", hdr)
    assert _capi.MAX_CARRIED_SPHERES == 256 and scoring.MAX_CARRIED_SPHERES == 256


def test_the_section_stands_behind_moving_obstacles():
    hdr = open(os.path.join(ROOT, "include", "gpmp2mi.h")).read()
    heads = re.findall(r"^/\* ---- ([a-z -]+?):", hdr, flags=re.M)
    k = heads.index("moving obstacles")
    assert heads[k + 1] == "carried object", heads[k:k + 3]


def test_null_negative_and_oversized_arguments_are_refused_before_any_device_work(eng):
    lib = eng.lib
    t = np.zeros((1, 3, 4))
    rad, cen = np.full(257, 0.1), np.zeros((257, 3))
    conf, err = np.zeros((1, 2)), np.zeros(8)
    one = C.c_void_p(1)   # a non-null handle that must never be looked at: the bad argument is reported first
    best, n = C.c_int(7), C.c_int(7)
    r_, c_, t_, q_, e_ = E.dptr(rad), E.dptr(cen), E.dptr(t), E.dptr(conf), E.dptr(err)
    none5 = (None,) * 5
    calls = {
        "set plan": lambda: lib.gpmp2mi_plan_set_carried(None, 0, 1, r_, c_),
        "set A < 0": lambda: lib.gpmp2mi_plan_set_carried(one, 0, -1, r_, c_),
        "set A > max": lambda: lib.gpmp2mi_plan_set_carried(one, 0, 257, r_, c_),
        "set radius": lambda: lib.gpmp2mi_plan_set_carried(one, 0, 1, None, c_),
        "set centers": lambda: lib.gpmp2mi_plan_set_carried(one, 0, 1, r_, None),
        "set_dev A > max": lambda: lib.gpmp2mi_plan_set_carried_dev(one, 0, 257, one, one, None),
        "set_dev radius": lambda: lib.gpmp2mi_plan_set_carried_dev(one, 0, 1, None, one, None),
        "set_dev plan": lambda: lib.gpmp2mi_plan_set_carried_dev(None, 0, 1, one, one, None),
        "factor robot": lambda: lib.gpmp2mi_carried_sphere_factor(None, one, 0, 1, r_, c_, 0.1, 1, q_, e_, None),
        "factor sdf": lambda: lib.gpmp2mi_carried_sphere_factor(one, None, 0, 1, r_, c_, 0.1, 1, q_, e_, None),
        "factor conf": lambda: lib.gpmp2mi_carried_sphere_factor(one, one, 0, 1, r_, c_, 0.1, 1, None, e_, None),
        "factor err": lambda: lib.gpmp2mi_carried_sphere_factor(one, one, 0, 1, r_, c_, 0.1, 1, q_, None, None),
        "factor M < 0": lambda: lib.gpmp2mi_carried_sphere_factor(one, one, 0, 1, r_, c_, 0.1, -1, q_, e_, None),
        "factor A < 0": lambda: lib.gpmp2mi_carried_sphere_factor(one, one, 0, -1, r_, c_, 0.1, 1, q_, e_, None),
        "factor A > max": lambda: lib.gpmp2mi_carried_sphere_factor(one, one, 0, 257, r_, c_, 0.1, 1, q_, e_, None),
        "factor radius": lambda: lib.gpmp2mi_carried_sphere_factor(one, one, 0, 1, None, c_, 0.1, 1, q_, e_, None),
        "score_traj traj": lambda: lib.gpmp2mi_carried_score_traj(one, one, 0, 1, r_, c_, 0.1, 0, 1, 2, None, *none5),
        "score_traj A > max": lambda: lib.gpmp2mi_carried_score_traj(one, one, 0, 257, r_, c_, 0.1, 0, 1, 2, t_, *none5),
        "score_traj centers": lambda: lib.gpmp2mi_carried_score_traj(one, one, 0, 1, r_, None, 0.1, 0, 1, 2, t_, *none5),
        "score_traj inter": lambda: lib.gpmp2mi_carried_score_traj(one, one, 0, 1, r_, c_, 0.1, -1, 1, 2, t_, *none5),
        "score_traj B": lambda: lib.gpmp2mi_carried_score_traj(one, one, 0, 1, r_, c_, 0.1, 0, -1, 2, t_, *none5),
        "score_traj N": lambda: lib.gpmp2mi_carried_score_traj(one, one, 0, 1, r_, c_, 0.1, 0, 1, 0, t_, *none5),
        "score_traj dt": lambda: lib.gpmp2mi_carried_score_traj(one, one, 0, 1, r_, c_, 0.0, 0, 1, 2, t_, *none5),
        "score_traj_dev A < 0": lambda: lib.gpmp2mi_carried_score_traj_dev(one, one, 0, -1, one, one, 0.1, 0, 1, 2, one, *none5, None),
        "score_traj robot": lambda: lib.gpmp2mi_carried_score_traj(None, one, 0, 1, r_, c_, 0.1, 0, 1, 2, t_, *none5),
        "score_traj sdf": lambda: lib.gpmp2mi_carried_score_traj(one, None, 0, 1, r_, c_, 0.1, 0, 1, 2, t_, *none5),
        "score_traj_dev robot": lambda: lib.gpmp2mi_carried_score_traj_dev(None, one, 0, 1, one, one, 0.1, 0, 1, 2, one, *none5, None),
        "score_traj_dev sdf": lambda: lib.gpmp2mi_carried_score_traj_dev(one, None, 0, 1, one, one, 0.1, 0, 1, 2, one, *none5, None),
        "plan_carried_score plan": lambda: lib.gpmp2mi_plan_carried_score(None, 0, *none5),
        "plan_carried_score_dev plan": lambda: lib.gpmp2mi_plan_carried_score_dev(None, 0, *none5, None),
        "select_carried plan": lambda: lib.gpmp2mi_plan_select_carried(None, 0, 0.0, 0, None, 0.0, 0.0, C.byref(best), C.byref(n), None, None),
        "select_carried_dev plan": lambda: lib.gpmp2mi_plan_select_carried_dev(None, 0, 0.0, 0, None, 0.0, 0.0, None, None, None, None, None),
    }
    for name, call in calls.items():
        assert call() == 1, name
        assert len(lib.gpmp2mi_last_error()) > 0, name
    assert (best.value, n.value) == (7, 7)      # a refused call writes nothing
    assert lib.gpmp2mi_plan_carried_count(None) == -1 and len(lib.gpmp2mi_last_error()) > 0


def test_graph_opts_default_leaves_the_new_fields_zero(eng):
    o = _capi.GraphOpts()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    eng.lib.gpmp2mi_graph_opts_default(C.byref(o))
    assert (o.max_carried_spheres, o.carried_first, o.carried_last) == (0, 0, 0)
    assert (o.carried_epsilon, o.carried_sigma) == (0.0, 0.0)
    assert o.lm_lambda_initial == 100.0 and o.workspace_path == 0
    # the new fields stand between self_collision and workspace_path, in the header's order
    names = [name for name, _ in _capi.GraphOpts._fields_]
    k = names.index("self_collision")
    assert names[k + 1:k + 7] == NEW_FIELDS + ["workspace_path"]
    fields = re.search(r"typedef struct gpmp2mi_graph_opts \{(.*?)\} gpmp2mi_graph_opts;", _header(), flags=re.S).group(1)
    order = [fields.index(w) for w in ["self_collision["] + [" " + x for x in NEW_FIELDS] + [" workspace_path;"]]
    assert order == sorted(order)


def test_graph_opts_mirror_has_the_size_and_offsets_of_the_header(tmp_path):
    probe = NEW_FIELDS + ["self_collision", "workspace_path", "max_self_pairs", "max_moving_spheres", "moving_sigma"]
    src = tmp_path / "opts_size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gpmp2mi.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(gpmp2mi_graph_opts));\n'
                   + "".join(f'  printf(" %zu", offsetof(gpmp2mi_graph_opts, {x}));\n' for x in probe)
                   + '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "opts_size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(_capi.GraphOpts)] + [getattr(_capi.GraphOpts, x).offset for x in probe]
    assert got == want, (got, want)


def test_settings_carry_the_capacity_the_range_and_the_constants():
    s = TrajOptimizerSetting(7)
    s.set_total_step(12)
    _, o, _ = _capi.make_settings(s)
    assert (o.max_carried_spheres, o.carried_first, o.carried_last, o.carried_epsilon, o.carried_sigma) == (0, 0, 0, 0.0, 0.0)
    s.set_carried_spheres(200, 0.05, 0.02)
    _, o, _ = _capi.make_settings(s)
    assert (o.max_carried_spheres, o.carried_first, o.carried_last, o.carried_epsilon, o.carried_sigma) == (200, 0, 12, 0.05, 0.02)
    s.set_carried_spheres(3, 0.1, 0.5, states=(1, 11))
    _, o, _ = _capi.make_settings(s)
    assert (o.max_carried_spheres, o.carried_first, o.carried_last) == (3, 1, 11)
    s.set_carried_spheres(257, 0.1, 0.5)
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
    r = s = Handle()
    good = np.zeros((2, 5, 14))
    rad, cen = np.full(2, 0.1), np.zeros((2, 3))
    for bad in (np.zeros((2, 4)), np.zeros((3, 3)), np.zeros(6)):
        with pytest.raises(ValueError):
            eng.carried_score_traj(r, s, 6, rad, bad, 0.1, 1, good)
    with pytest.raises(ValueError):
        eng.carried_score_traj(r, s, 6, np.full(257, 0.1), np.zeros((257, 3)), 0.1, 1, good)
    with pytest.raises(ValueError):
        eng.carried_score_traj(r, s, 6, rad, cen, 0.1, -1, good)
    with pytest.raises(ValueError):
        eng.carried_score_traj(r, s, 6, rad, cen, 0.0, 1, good)
    for out in ({"worst": np.zeros((2, 3), dtype=np.int32)}, {"dense_cost": np.zeros(2)}, {"out_of_range": np.zeros(2)}):
        with pytest.raises(ValueError):
            eng.carried_score_traj(r, s, 6, rad, cen, 0.1, 1, good, out=out)
    with pytest.raises(ValueError):
        eng.carried_sphere_factor(r, s, 6, np.full(257, 0.1), np.zeros((257, 3)), 0.1, np.zeros((1, 7)))
    pl = E.Plan.__new__(E.Plan)
    pl.eng, pl.B, pl.N, pl.D = eng, 2, 4, 7
    with pytest.raises(ValueError):
        pl.set_carried(6, rad, np.zeros((2, 4)))
    with pytest.raises(ValueError):
        pl.carried_score(-1)
    with pytest.raises(ValueError):
        pl.carried_score(1, out={"carried_dense_cost": np.zeros(5)})
    with pytest.raises(ValueError):
        pl.select_carried(-2)
    with pytest.raises(ValueError):
        pl.select_carried_dev(-2)
