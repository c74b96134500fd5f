"""Workspace path (include/gpmp2mi.h "workspace path") as far as it can be checked without a GPU: the ABI is declared and
exported, argument errors are reported before any device work, gpmp2mi_graph_opts and its ctypes mirror agree, the
selection rule and the straight-line path of gpmp2_amd.scoring on hand cases.  What needs a live plan is in
tests/test_gpu_path.py."""
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
INT_NAMES = ["gpmp2mi_plan_set_workspace_path", "gpmp2mi_plan_set_workspace_path_dev", "gpmp2mi_workspace_path_factor",
             "gpmp2mi_path_score_traj", "gpmp2mi_path_score_traj_dev", "gpmp2mi_plan_path_score",
             "gpmp2mi_plan_path_score_dev", "gpmp2mi_plan_select_path", "gpmp2mi_plan_select_path_dev"]
NEW_FIELDS = ["workspace_path", "workspace_path_mode", "workspace_path_link"]


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def test_entry_points_are_declared_and_exported(eng):
    hdr = open(os.path.join(ROOT, "include", "gpmp2mi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in INT_NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr), f"{n} is not declared in include/gpmp2mi.h"
        assert hasattr(eng.lib, n), f"{n} is not exported"
        assert getattr(eng.lib, n).argtypes is not None, f"{n} has no argtypes (_capi.declare_path)"


def test_null_and_bad_arguments_are_refused_before_any_device_work(eng):
    lib = eng.lib
    t, des, sg = np.zeros((1, 3, 4)), np.tile(np.eye(4), (3, 1, 1)), np.full(3, 0.1)
    conf, err = np.zeros((1, 2)), np.zeros(6)
    one = C.c_void_p(1)   # a non-null handle that must never be looked at: the bad argument is reported first
    best, n = C.c_int(7), C.c_int(7)
    d_, s_, t_ = E.dptr(des), E.dptr(sg), E.dptr(t)
    none6 = (None,) * 6
    calls = {
        "set plan": lambda: lib.gpmp2mi_plan_set_workspace_path(None, d_, s_),
        "set_dev plan": lambda: lib.gpmp2mi_plan_set_workspace_path_dev(None, one, one, None),
        "factor robot": lambda: lib.gpmp2mi_workspace_path_factor(None, 0, 0, 1, E.dptr(conf), d_, E.dptr(err), None),
        "factor conf": lambda: lib.gpmp2mi_workspace_path_factor(one, 0, 0, 1, None, d_, E.dptr(err), None),
        "factor des": lambda: lib.gpmp2mi_workspace_path_factor(one, 0, 0, 1, E.dptr(conf), None, E.dptr(err), None),
        "factor err": lambda: lib.gpmp2mi_workspace_path_factor(one, 0, 0, 1, E.dptr(conf), d_, None, None),
        "factor M < 0": lambda: lib.gpmp2mi_workspace_path_factor(one, 0, 0, -1, E.dptr(conf), d_, E.dptr(err), None),
        "factor mode": lambda: lib.gpmp2mi_workspace_path_factor(one, 3, 0, 1, E.dptr(conf), d_, E.dptr(err), None),
        "score_traj robot": lambda: lib.gpmp2mi_path_score_traj(None, 0, 0, d_, s_, 0.1, 0, 1, 2, t_, *none6),
        "score_traj traj": lambda: lib.gpmp2mi_path_score_traj(one, 0, 0, d_, s_, 0.1, 0, 1, 2, None, *none6),
        "score_traj des": lambda: lib.gpmp2mi_path_score_traj(one, 0, 0, None, s_, 0.1, 0, 1, 2, t_, *none6),
        "score_traj sigma": lambda: lib.gpmp2mi_path_score_traj(one, 0, 0, d_, None, 0.1, 0, 1, 2, t_, *none6),
        "score_traj mode": lambda: lib.gpmp2mi_path_score_traj(one, -1, 0, d_, s_, 0.1, 0, 1, 2, t_, *none6),
        "score_traj_dev robot": lambda: lib.gpmp2mi_path_score_traj_dev(None, 0, 0, one, one, 0.1, 0, 1, 2, one, *none6, None),
        "score_traj_dev traj": lambda: lib.gpmp2mi_path_score_traj_dev(one, 0, 0, one, one, 0.1, 0, 1, 2, None, *none6, None),
        "score_traj_dev mode": lambda: lib.gpmp2mi_path_score_traj_dev(one, 3, 0, one, one, 0.1, 0, 1, 2, one, *none6, None),
        "plan_path_score plan": lambda: lib.gpmp2mi_plan_path_score(None, 0, *none6),
        "plan_path_score_dev plan": lambda: lib.gpmp2mi_plan_path_score_dev(None, 0, *none6, None),
        "select_path plan": lambda: lib.gpmp2mi_plan_select_path(None, 0, 0.0, 0, 1.0, 1.0, C.byref(best), C.byref(n), None, None),
        "select_path_dev plan": lambda: lib.gpmp2mi_plan_select_path_dev(None, 0, 0.0, 0, 1.0, 1.0, None, None, None, None, None),
    }
    for name, call in calls.items():
        assert call() == 1, name
        assert len(lib.gpmp2mi_last_error()) > 0, name
    assert (best.value, n.value) == (7, 7)      # a refused call writes nothing


def test_graph_opts_default_leaves_the_new_fields_zero(eng):
    o = _capi.GraphOpts()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    eng.lib.gpmp2mi_graph_opts_default(C.byref(o))
    assert (o.workspace_path, o.workspace_path_mode, o.workspace_path_link) == (0, 0, 0)
    assert o.lm_lambda_initial == 100.0 and o.max_moving_spheres == 0
    names = [name for name, _ in _capi.GraphOpts._fields_]
    assert names[names.index("workspace_path"):][:3] == NEW_FIELDS


def test_graph_opts_mirror_has_the_size_and_offsets_of_the_header(tmp_path):
    fields = NEW_FIELDS + ["self_collision", "max_moving_spheres", "moving_sigma"]
    src = tmp_path / "opts_size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gpmp2mi.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(gpmp2mi_graph_opts));\n'
                   + "".join(f'  printf(" %zu", offsetof(gpmp2mi_graph_opts, {f}));\n' for f in fields)
                   + '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "opts_size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(_capi.GraphOpts)] + [getattr(_capi.GraphOpts, f).offset for f in fields]
    assert got == want, (got, want)


def test_settings_carry_the_mode_and_the_link():
    s = TrajOptimizerSetting(7)
    s.set_total_step(12)
    _, o, _ = _capi.make_settings(s)
    assert (o.workspace_path, o.workspace_path_mode, o.workspace_path_link) == (0, 0, 0)
    s.set_workspace_path(_capi.WORKSPACE_POSE, 6)
    _, o, _ = _capi.make_settings(s)
    assert (o.workspace_path, o.workspace_path_mode, o.workspace_path_link) == (1, 2, 6)
    s.set_workspace_path(3, 6)
    with pytest.raises(ValueError):
        _capi.make_settings(s)


def test_path_rule_on_hand_cases():
    fe = np.array([3.0, 1.0, 1.0, 0.5, np.nan])
    st = np.array([0, 0, 0, 3, 0])
    clr, oor = np.array([0.1, 0.1, 0.1, 0.1, 0.1]), np.zeros(5, dtype=np.int32)
    pos, rot, inv = np.array([0.01, 0.03, 0.01, 0.0, 0.0]), np.array([0.1, 0.1, 0.3, 0.0, 0.0]), np.array([0, 0, 0, 0, 0])
    # no path condition: the rule of select_rule (row 3 is not SPD, row 4 not finite; the tie goes to the lower row)
    assert scoring.path_rule(fe, st, clr, oor) == scoring.select_rule(fe, st, clr, oor) == (1, 3)
    assert scoring.path_rule(fe, st, clr, oor, max_pos_dev=pos, max_rot_dev=rot, path_invalid=inv) == (1, 3)
    assert scoring.path_rule(fe, st, clr, oor, max_pos_dev=pos, max_pos_dev_allowed=0.02) == (2, 2)
    assert scoring.path_rule(fe, st, clr, oor, max_pos_dev=pos, max_rot_dev=rot, max_pos_dev_allowed=0.02,
                             max_rot_dev_allowed=0.2) == (0, 1)
    assert scoring.path_rule(fe, st, clr, oor, max_pos_dev=pos, max_pos_dev_allowed=0.01) == (2, 2)      # <=, not <
    assert scoring.path_rule(fe, st, clr, oor, max_pos_dev=pos, max_pos_dev_allowed=0.005) == (-1, 0)
    assert scoring.path_rule(fe, st, clr, oor, path_invalid=np.array([0, 1, 0, 0, 0])) == (2, 2)
    assert scoring.path_rule(fe, st, clr, oor, max_pos_dev=np.full(5, np.nan), max_pos_dev_allowed=np.inf) == (-1, 0)
    assert scoring.path_rule(fe, st, clr, oor, required_clearance=0.2) == (-1, 0)


def test_line_path_end_poses_are_exact():
    rng = np.random.default_rng(0)
    A, B = np.eye(4), np.eye(4)
    A[:3, :3], _ = np.linalg.qr(rng.normal(size=(3, 3)))
    B[:3, :3], _ = np.linalg.qr(rng.normal(size=(3, 3)))
    A[:3, :3] *= np.sign(np.linalg.det(A[:3, :3]))
    B[:3, :3] *= np.sign(np.linalg.det(B[:3, :3]))
    A[:3, 3], B[:3, 3] = rng.normal(size=3), rng.normal(size=3)
    des = scoring.line_path(A, B, 7)
    assert des.shape == (8, 4, 4)
    assert np.array_equal(des[0], A) and np.array_equal(des[7], B)
    for i in range(8):
        R = des[i, :3, :3]
        np.testing.assert_allclose(R.T @ R, np.eye(3), atol=1e-14)
        np.testing.assert_allclose(des[i, :3, 3], A[:3, 3] + i / 7.0 * (B[:3, 3] - A[:3, 3]), atol=1e-15)
        assert np.array_equal(des[i, 3], [0.0, 0.0, 0.0, 1.0])
    # equal angular steps along the geodesic
    steps = [np.arccos(np.clip((np.trace(des[i, :3, :3].T @ des[i + 1, :3, :3]) - 1.0) / 2.0, -1.0, 1.0)) for i in range(7)]
    np.testing.assert_allclose(steps, steps[0], rtol=1e-7)
    with pytest.raises(ValueError):
        scoring.line_path(A, B, 0)
    # an eased profile: the same line, the states elsewhere on it
    u = np.arange(8) / 7.0
    eased = scoring.line_path(A, B, 7, s=3 * u ** 2 - 2 * u ** 3)
    assert np.array_equal(eased[0], A) and np.array_equal(eased[7], B)
    np.testing.assert_allclose(eased[1, :3, 3], A[:3, 3] + (3 * u[1] ** 2 - 2 * u[1] ** 3) * (B[:3, 3] - A[:3, 3]), atol=1e-15)
    with pytest.raises(ValueError):
        scoring.line_path(A, B, 7, s=u[:7])


def test_python_wrappers_refuse_bad_input_before_the_library_is_called():
    class Boom:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name})")

    class Handle:
        ptr, dof, S = None, 7, 16

    eng = E.Engine.__new__(E.Engine)
    eng.lib = Boom()
    r = Handle()
    good, des = np.zeros((2, 5, 14)), np.tile(np.eye(4), (5, 1, 1))
    for bad in (np.zeros((4, 4, 4)), np.zeros((5, 3, 4)), np.zeros((5, 15))):
        with pytest.raises(ValueError):
            eng.path_score_traj(r, 0, 6, bad, 0.1, 0.1, 1, good)
    with pytest.raises(ValueError):
        eng.path_score_traj(r, 0, 6, des, np.full(4, 0.1), 0.1, 1, good)
    with pytest.raises(ValueError):
        eng.path_score_traj(r, 0, 6, des, 0.1, 0.1, -1, good)
    with pytest.raises(ValueError):
        eng.path_score_traj(r, 0, 6, des, 0.1, 0.0, 1, good)
    for out in ({"worst": np.zeros((2, 3), dtype=np.int32)}, {"clearance": np.zeros(2)}, {"invalid": np.zeros(2)}):
        with pytest.raises(ValueError):
            eng.path_score_traj(r, 0, 6, des, 0.1, 0.1, 1, good, out=out)
    pl = E.Plan.__new__(E.Plan)
    pl.eng, pl.B, pl.N, pl.D = eng, 2, 4, 7
    with pytest.raises(ValueError):
        pl.set_workspace_path(np.zeros((4, 4, 4)), 0.1)
    with pytest.raises(ValueError):
        pl.set_workspace_path(des)
    with pytest.raises(ValueError):
        pl.path_score(-1)
    with pytest.raises(ValueError):
        pl.path_score(1, out={"dense_cost": np.zeros(5)})
    with pytest.raises(ValueError):
        pl.select_path(-2)
    with pytest.raises(ValueError):
        pl.select_path_dev(-2)
