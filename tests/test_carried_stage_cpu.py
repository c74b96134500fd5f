"""stages.CARRIED (gpmp2_amd/stages.py) against include/gpmp2mi.h, as tests/test_stage_table_cpu.py holds the stages of
the STAGES dict: the four score entry points of the carried object end in the table's outputs, in order and with the
table's types; scoring.CARRIED_NAMES is the table; the STAGES dict is what it was.  No GPU and no library."""
import numpy as np
import pytest

from gpmp2_amd import scoring, stages

from test_stage_table_cpu import header_params

ENTRY_POINTS = ["gpmp2mi_carried_score_traj", "gpmp2mi_carried_score_traj_dev", "gpmp2mi_plan_carried_score",
                "gpmp2mi_plan_carried_score_dev"]


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_every_entry_point_ends_in_the_tables_outputs(fn):
    pars = header_params(fn)
    if pars[-1] == ("void*", "stream"):
        pars = pars[:-1]
    want = [("int*" if dt is np.int32 else "double*", name) for name, dt, _ in stages.CARRIED.outputs]
    assert pars[-len(want):] == want, fn


def test_the_names_tuple_is_the_table():
    assert isinstance(scoring.CARRIED_NAMES, tuple) and scoring.CARRIED_NAMES == stages.names(stages.CARRIED)
    assert scoring.CARRIED_NAMES == ("carried_support_cost", "carried_dense_cost", "min_carried_clearance", "worst",
                                     "out_of_range")
    assert stages.CARRIED.word == "score" and not stages.CARRIED.absent
    sh = {n: s for n, _, s in stages.shapes(stages.CARRIED, 3, 5, 2)}
    assert sh["worst"] == (3, 2) and sh["min_carried_clearance"] == (3,)


def test_the_stages_dict_is_what_it_was():
    assert list(stages.STAGES) == ["score", "self", "moving", "path", "motion", "torque", "retime"]
    assert all(s is not stages.CARRIED for s in stages.STAGES.values())


def test_the_rule_adds_two_conditions():
    fe, st = np.array([3.0, 1.0, 2.0, 0.5]), np.zeros(4, dtype=np.int32)
    clr, oor = np.full(4, 1.0), np.zeros(4, dtype=np.int32)
    cc, coor = np.array([0.2, -0.1, 0.3, np.inf]), np.array([0, 0, 0, 4], dtype=np.int32)
    assert scoring.carried_rule(fe, st, clr, oor) == scoring.select_rule(fe, st, clr, oor)
    assert scoring.carried_rule(fe, st, clr, oor, min_carried_clearance=cc, carried_out_of_range=coor,
                                required_carried_clearance=0.0) == (3, 3)
    assert scoring.carried_rule(fe, st, clr, oor, 0.0, True, min_carried_clearance=cc, carried_out_of_range=coor,
                                required_carried_clearance=0.0) == (2, 2)
    assert scoring.carried_rule(fe, st, clr, oor, min_carried_clearance=cc, carried_out_of_range=coor,
                                required_carried_clearance=1.0) == (3, 1)
