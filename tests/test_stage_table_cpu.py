"""The table of the check stages (gpmp2_amd/stages.py) against include/gpmp2mi.h: every entry point of a stage ends in the
table's outputs, in order and with the table's types, and scoring's *_NAMES tuples are the table's names.  No GPU and no
library."""
import os
import re

import numpy as np
import pytest

from gpmp2_amd import scoring, stages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_params(name):
    """[(type, name)] of `int name(...)` in include/gpmp2mi.h, comments stripped"""
    hdr = open(os.path.join(ROOT, "include", "gpmp2mi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/gpmp2mi.h"
    pars = []
    for par in m.group(1).split(","):
        typ, _, ident = " ".join(par.split()).rpartition(" ")
        pars.append((typ, ident))
    return pars


def entry_points(key):
    """(function, names of `absent` the form drops) for every entry point of the stage"""
    if key == "retime":
        return [("gpmp2mi_retime_traj", ()), ("gpmp2mi_retime_traj_dev", ()), ("gpmp2mi_plan_retime", ()),
                ("gpmp2mi_plan_retime_dev", ()), ("gpmp2mi_retime_path", ("dense_retimed",))]
    return [(f"gpmp2mi_{key}{'_score' if key != 'score' else ''}_traj{dev}", ()) for dev in ("", "_dev")] + \
           [(f"gpmp2mi_plan_{key}{'_score' if key != 'score' else ''}{dev}", ()) for dev in ("", "_dev")]


def test_there_is_one_entry_per_stage():
    assert list(stages.STAGES) == ["score", "self", "moving", "path", "motion", "torque", "retime"]
    assert [stages.STAGES[k].word for k in stages.STAGES] == ["score", "score", "score", "path", "motion", "torque", "retime"]
    assert stages.TORQUE.absent == {"tau": "null"} and stages.RETIME.absent == {"dense_retimed": "dropped"}
    assert all(not stages.STAGES[k].absent for k in ("score", "self", "moving", "path", "motion"))


@pytest.mark.parametrize("key", list(stages.STAGES))
def test_every_entry_point_ends_in_the_tables_outputs(key):
    stage = stages.STAGES[key]
    for fn, dropped in entry_points(key):
        pars = header_params(fn)
        if pars[-1] == ("void*", "stream"):
            pars = pars[:-1]
        want = [("int*" if dt is np.int32 else "double*", name) for name, dt, _ in stage.outputs if name not in dropped]
        assert all(dt in (np.int32, np.float64) for _, dt, _ in stage.outputs)
        assert pars[-len(want):] == want, fn
        assert stage.absent.get(dropped[0]) == "dropped" if dropped else True


def test_the_names_tuples_are_the_tables():
    for key, tup in (("score", scoring.SCORE_NAMES), ("self", scoring.SELF_NAMES), ("moving", scoring.MOVING_NAMES),
                     ("path", scoring.PATH_NAMES), ("motion", scoring.MOTION_NAMES), ("torque", scoring.TORQUE_NAMES),
                     ("retime", scoring.RETIME_NAMES)):
        assert isinstance(tup, tuple) and tup == stages.names(stages.STAGES[key]), key


def test_shapes_follow_md_and_d():
    B, Md, D = 3, 5, 2
    sh = {k: {n: s for n, _, s in stages.shapes(stages.STAGES[k], B, Md, D)} for k in stages.STAGES}
    assert sh["score"]["worst"] == (B, 2) and sh["moving"]["worst"] == (B, 3) and sh["motion"]["worst"] == (B, 4, 2)
    assert sh["torque"]["worst"] == (B, 3, 2) and sh["torque"]["tau"] == (B, Md, D)
    assert sh["retime"]["stamps"] == (B, Md) and sh["retime"]["achieved"] == (B, 4)
    assert sh["retime"]["dense_retimed"] == (B, Md, 2 * D) and sh["path"]["max_pos_dev"] == (B,)
    path_form = stages.shapes(stages.RETIME, B, Md, None, absent=("dense_retimed",))
    assert [n for n, _, _ in path_form] == list(scoring.RETIME_NAMES[:-1])


def test_the_validator_keeps_its_messages():
    o = stages.outputs(stages.TORQUE, 2, 5, 2, absent=("tau",))
    assert list(o) == list(scoring.TORQUE_NAMES) and o["tau"] is None and o["worst"].dtype == np.int32
    tau = np.zeros((2, 5, 2))
    assert stages.outputs(stages.TORQUE, 2, 5, 2, dict(tau=tau), absent=("tau",))["tau"] is tau
    for key in stages.STAGES:
        with pytest.raises(ValueError, match=rf"unknown {stages.STAGES[key].word} outputs: \['nope'\]"):
            stages.outputs(stages.STAGES[key], 2, 5, 2, dict(nope=None))
    with pytest.raises(ValueError, match="unknown retime outputs: \\['dense_retimed'\\]"):
        stages.outputs(stages.RETIME, 2, 5, None, dict(dense_retimed=np.zeros((2, 5, 4))), absent=("dense_retimed",))
    with pytest.raises(ValueError, match=r"worst: expected a contiguous int32 array of shape \[2, 4, 2\], got float64 \[2, 4, 2\]"):
        stages.outputs(stages.MOTION, 2, out=dict(worst=np.zeros((2, 4, 2))))
