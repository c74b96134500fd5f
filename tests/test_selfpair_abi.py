"""The self-collision table of a plan (include/gpmp2mi.h "self-collision table in a plan") as far as it can be checked
without a GPU: the two calls are declared and exported, gpmp2mi_graph_opts grew between the workspace-path and the
moving-sphere fields and its ctypes mirror has the header's size and offsets, the settings reach the struct, and a NULL
plan is refused.  What needs a live plan is in tests/test_gpu_selfpair.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

from gpmp2_amd import _capi
from gpmp2_amd import engine as E
from gpmp2_amd.settings import TrajOptimizerSetting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_NAMES = ["gpmp2mi_plan_set_self_pairs", "gpmp2mi_plan_self_pairs_count"]
NEW_FIELDS = ["max_self_pairs", "self_pairs_first", "self_pairs_last"]


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def _probe(tmp_path, body):
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gpmp2mi.h"\nint main(void) {\n' + body
                   + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]


def test_entry_points_are_declared_and_exported(eng):
    hdr = open(os.path.join(ROOT, "include", "gpmp2mi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in INT_NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr), f"{n} is not declared in include/gpmp2mi.h"
        assert hasattr(eng.lib, n), f"{n} is not exported"
        assert getattr(eng.lib, n).argtypes is not None and getattr(eng.lib, n).restype is C.c_int
    assert eng.lib.gpmp2mi_plan_set_self_pairs.argtypes == [C.c_void_p, C.c_void_p]
    assert eng.lib.gpmp2mi_plan_self_pairs_count.argtypes == [C.c_void_p]


def test_the_maximum_is_all_pairs_of_the_largest_sphere_model(tmp_path):
    got = _probe(tmp_path, '  printf("%d %d\\n", GPMP2MI_MAX_SPHERES, GPMP2MI_MAX_PLAN_SELF_PAIRS);\n')
    assert got[1] == got[0] * (got[0] - 1) // 2
    assert _capi.MAX_PLAN_SELF_PAIRS == got[1]


def test_the_new_fields_stand_between_the_path_and_the_moving_fields():
    names = [name for name, _ in _capi.GraphOpts._fields_]
    k = names.index("workspace_path_link")
    assert names[k + 1:k + 5] == NEW_FIELDS + ["max_moving_spheres"]


def test_graph_opts_default_leaves_the_new_fields_zero(eng):
    o = _capi.GraphOpts()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    eng.lib.gpmp2mi_graph_opts_default(C.byref(o))
    assert (o.max_self_pairs, o.self_pairs_first, o.self_pairs_last) == (0, 0, 0)
    assert o.lm_lambda_initial == 100.0 and o.max_moving_spheres == 0 and o.workspace_path == 0


def test_graph_opts_mirror_has_the_size_and_offsets_of_the_header(tmp_path):
    fields = ["workspace_path_link"] + NEW_FIELDS + ["max_moving_spheres", "moving_sigma"]
    got = _probe(tmp_path, '  printf("%zu", sizeof(gpmp2mi_graph_opts));\n'
                 + "".join(f'  printf(" %zu", offsetof(gpmp2mi_graph_opts, {f}));\n' for f in fields))
    want = [C.sizeof(_capi.GraphOpts)] + [getattr(_capi.GraphOpts, f).offset for f in fields]
    assert got == want, (got, want)


def test_settings_carry_the_capacity_and_the_range():
    s = TrajOptimizerSetting(7)
    s.set_total_step(12)
    _, o, _ = _capi.make_settings(s)
    assert (o.max_self_pairs, o.self_pairs_first, o.self_pairs_last) == (0, 0, 0)
    s.set_self_pairs(78)
    _, o, _ = _capi.make_settings(s)
    assert (o.max_self_pairs, o.self_pairs_first, o.self_pairs_last) == (78, 0, 12)
    s.set_self_pairs(1200, states=(1, 11))
    _, o, _ = _capi.make_settings(s)
    assert (o.max_self_pairs, o.self_pairs_first, o.self_pairs_last) == (1200, 1, 11)
    s.set_self_pairs(_capi.MAX_PLAN_SELF_PAIRS)
    _capi.make_settings(s)
    for bad in (_capi.MAX_PLAN_SELF_PAIRS + 1, -1):
        s.set_self_pairs(bad)
        with pytest.raises(ValueError):
            _capi.make_settings(s)


def test_a_null_plan_is_refused(eng):
    lib = eng.lib
    one = C.c_void_p(1)   # a non-null table that must never be looked at
    assert lib.gpmp2mi_plan_set_self_pairs(None, one) == 1
    assert len(lib.gpmp2mi_last_error()) > 0
    assert lib.gpmp2mi_plan_set_self_pairs(None, None) == 1
    assert lib.gpmp2mi_plan_self_pairs_count(None) == -1
