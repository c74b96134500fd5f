"""The score-and-select stage (include/gpmp2mi.h "scoring") as far as it can be checked without a GPU: the ABI is
declared and exported, argument errors are reported before any device work, the selection rule (gpmp2_amd.scoring
states it in numpy, gpmp2mi_select_best runs it on the host) and, on the CPU oracle alone, the fact the stage exists
for: a trajectory whose support states are collision-free can collide between them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import score_reference as ref
from gpmp2_amd import engine as E
from gpmp2_amd import scoring

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gpmp2mi_score_traj", "gpmp2mi_score_traj_dev", "gpmp2mi_select_best", "gpmp2mi_select_best_dev",
         "gpmp2mi_plan_score", "gpmp2mi_plan_score_dev", "gpmp2mi_plan_select", "gpmp2mi_plan_select_dev",
         "gpmp2mi_multi_plan_score", "gpmp2mi_multi_plan_select"]


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def test_scoring_entry_points_are_declared_and_exported(eng):
    hdr = open(os.path.join(ROOT, "include", "gpmp2mi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr), f"{n} is not declared in include/gpmp2mi.h"
        assert hasattr(eng.lib, n), f"{n} is not exported"


def test_null_handles_are_refused_before_any_device_work(eng):
    lib = eng.lib
    t = np.zeros((1, 3, 4))
    fe, clr = np.zeros(2), np.zeros(2)
    one = C.c_void_p(1)   # a non-null handle that must never be looked at: the null one is reported first
    best, n = C.c_int(7), C.c_int(7)
    calls = {
        "plan_score": lambda: lib.gpmp2mi_plan_score(None, 0, None, None, None, None, None),
        "plan_score_dev": lambda: lib.gpmp2mi_plan_score_dev(None, 0, None, None, None, None, None, None),
        "plan_select": lambda: lib.gpmp2mi_plan_select(None, 0, 0.0, 0, None, None, None, None),
        "plan_select_dev": lambda: lib.gpmp2mi_plan_select_dev(None, 0, 0.0, 0, None, None, None, None, None),
        "multi_plan_score": lambda: lib.gpmp2mi_multi_plan_score(None, 0, None, None, None, None, None),
        "multi_plan_select": lambda: lib.gpmp2mi_multi_plan_select(None, 0, 0.0, 0, None, None, None, None),
        "score_traj robot": lambda: lib.gpmp2mi_score_traj(None, one, 0.1, 0, 1, 2, E.dptr(t), None, None, None, None, None),
        "score_traj sdf": lambda: lib.gpmp2mi_score_traj(one, None, 0.1, 0, 1, 2, E.dptr(t), None, None, None, None, None),
        "score_traj_dev robot": lambda: lib.gpmp2mi_score_traj_dev(None, one, 0.1, 0, 1, 2, one, None, None, None, None, None, None),
        "score_traj_dev sdf": lambda: lib.gpmp2mi_score_traj_dev(one, None, 0.1, 0, 1, 2, one, None, None, None, None, None, None),
        "select_best final_error": lambda: lib.gpmp2mi_select_best(2, None, None, E.dptr(clr), None, 0.0, 0, C.byref(best), C.byref(n)),
        "select_best B": lambda: lib.gpmp2mi_select_best(-1, E.dptr(fe), None, E.dptr(clr), None, 0.0, 0, C.byref(best), C.byref(n)),
        "select_best_dev final_error": lambda: lib.gpmp2mi_select_best_dev(2, None, None, one, None, 0.0, 0, None, None, None),
        "select_best_dev B": lambda: lib.gpmp2mi_select_best_dev(-1, one, None, one, None, 0.0, 0, None, None, None),
    }
    for name, call in calls.items():
        assert call() == 1, name
        assert len(lib.gpmp2mi_last_error()) > 0, name
    assert (best.value, n.value) == (7, 7)      # a refused call writes nothing


def test_python_wrappers_refuse_misshaped_arrays_before_the_library_is_called():
    class Boom:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name})")

    class Handle:
        ptr, dof = None, 7

    eng = E.Engine.__new__(E.Engine)
    eng.lib = Boom()
    r, s = Handle(), Handle()
    for bad in (np.zeros((2, 5, 13)), np.zeros((2, 5)), np.zeros(14), np.zeros((2, 3, 5, 14)), np.zeros((2, 1, 14))):
        with pytest.raises(ValueError):
            eng.score_traj(r, s, 0.1, 2, bad)
    good = np.zeros((2, 5, 14))
    with pytest.raises(ValueError):
        eng.score_traj(r, s, 0.1, -1, good)
    with pytest.raises(ValueError):
        eng.score_traj(r, s, 0.0, 1, good)
    for out in ({"dense_cost": np.zeros(3)}, {"worst": np.zeros((2, 2))}, {"out_of_range": np.zeros(2)},
                {"min_clearance": np.zeros((2, 1))}, {"support_cost": np.zeros(4)[::2]}, {"nonsense": np.zeros(2)}):
        with pytest.raises(ValueError):
            eng.score_traj(r, s, 0.1, 1, good, out=out)
    with pytest.raises(ValueError):
        eng.select_best(np.zeros(3), None, np.zeros(2))
    with pytest.raises(ValueError):
        eng.select_best(np.zeros(3), np.zeros(4, dtype=np.int32), np.zeros(3))
    with pytest.raises(ValueError):
        eng.select_best(np.zeros(3), None, np.zeros(3), out_of_range=None, require_in_range=True)
    pl = E.Plan.__new__(E.Plan)
    pl.eng, pl.B, pl.N, pl.D = eng, 2, 4, 7
    with pytest.raises(ValueError):
        pl.score(1, out={"dense_cost": np.zeros(5)})
    with pytest.raises(ValueError):
        pl.score(-1)
    with pytest.raises(ValueError):
        pl.select(-2)


INF, NAN = float("inf"), float("nan")


def test_select_rule_on_hand_written_cases():
    sel = scoring.select_rule
    ok = np.zeros(4, dtype=np.int32)
    # lowest error among the eligible
    assert sel([3.0, 1.0, 2.0, 5.0], ok, [0.1] * 4, [0] * 4) == (1, 4)
    # a cheaper row that is NOT_SPD / non-finite / below the clearance / out of range is skipped
    assert sel([3.0, 1.0, 2.0, 5.0], [0, 3, 0, 0], [0.1] * 4, [0] * 4) == (2, 3)
    assert sel([3.0, NAN, 2.0, -INF], ok, [0.1] * 4, [0] * 4) == (2, 2)
    assert sel([3.0, 1.0, 2.0, 5.0], ok, [0.1, -0.01, 0.1, 0.1], [0] * 4) == (2, 3)
    assert sel([3.0, 1.0, 2.0, 5.0], ok, [0.1, 0.04, 0.1, 0.1], [0] * 4, required_clearance=0.05) == (2, 3)
    assert sel([3.0, 1.0, 2.0, 5.0], ok, [0.1] * 4, [0, 2, 0, 0], require_in_range=True) == (2, 3)
    assert sel([3.0, 1.0, 2.0, 5.0], ok, [0.1] * 4, [0, 2, 0, 0], require_in_range=False) == (1, 4)
    # every status but NOT_SPD is fine; status None = all fine
    assert sel([5.0, 4.0, 3.0, 2.0, 1.0], [0, 1, 2, 3, 4], [0.1] * 5, [0] * 5) == (4, 4)
    assert sel([3.0, 1.0], None, [0.1, 0.1], None) == (1, 2)
    # exact ties go to the lowest row
    assert sel([2.0, 1.0, 1.0, 1.0], ok, [0.1] * 4, [0] * 4) == (1, 4)
    assert sel([2.0, 1.0, 1.0, 1.0], ok, [0.1, -1.0, 0.1, 0.1], [0] * 4) == (2, 3)
    # nothing eligible
    assert sel([1.0, 2.0], [3, 3], [0.1, 0.1], [0, 0]) == (-1, 0)
    assert sel([], None, [], []) == (-1, 0)
    # +inf clearance = nothing in range: eligible only without require_in_range
    assert sel([1.0, 2.0], None, [INF, 0.1], [8, 0], require_in_range=False) == (0, 2)
    assert sel([1.0, 2.0], None, [INF, 0.1], [8, 0], require_in_range=True) == (1, 1)
    # a NaN clearance never, not even at required_clearance = -inf; -inf admits every other clearance
    assert sel([1.0, 2.0], None, [NAN, -3.0], [0, 0], required_clearance=-INF) == (1, 1)
    assert sel([1.0, 2.0], None, [NAN, -3.0], [0, 0], required_clearance=0.0) == (-1, 0)


def test_library_select_best_agrees_with_the_rule(eng):
    cases = [([3.0, 1.0, 2.0, 5.0], [0, 3, 0, 0], [0.1] * 4, [0] * 4, 0.0, 0),
             ([2.0, 1.0, 1.0, 1.0], [0, 0, 0, 0], [0.1, -1.0, 0.1, 0.1], [0] * 4, 0.0, 0),
             ([1.0, 2.0], [0, 0], [INF, 0.1], [8, 0], 0.0, 1),
             ([1.0, 2.0], [0, 0], [NAN, -3.0], [0, 0], -INF, 0),
             ([1.0, 2.0], [3, 3], [0.1, 0.1], [0, 0], 0.0, 0)]
    for fe, st, clr, oor, req, rir in cases:
        assert eng.select_best(fe, st, clr, oor, req, bool(rir)) == scoring.select_rule(fe, st, clr, oor, req, bool(rir))
    assert eng.select_best([3.0, 1.0], None, [0.1, 0.1]) == (1, 2)              # status / out_of_range NULL
    assert eng.select_best([], None, []) == (-1, 0)                              # B = 0
    rng = np.random.default_rng(20260)
    values = np.array([0.5, 1.0, 1.5, 2.0, 2.5, 3.0, NAN, INF])
    clears = np.array([-0.2, -0.05, 0.0, 0.03, 0.08, 0.3, INF, -INF, NAN])
    for trial in range(200):
        B = int(rng.integers(1, 301))
        fe = rng.choice(values, size=B)
        st = rng.integers(0, 5, size=B).astype(np.int32)
        clr = rng.choice(clears, size=B, p=[0.15, 0.15, 0.1, 0.15, 0.15, 0.15, 0.05, 0.05, 0.05])
        oor = (rng.integers(0, 4, size=B) == 0).astype(np.int32) * rng.integers(1, 9, size=B).astype(np.int32)
        req = float(rng.choice([0.0, 0.05, -0.1, -INF]))
        rir = bool(rng.integers(0, 2))
        got = eng.select_best(fe, st, clr, oor, req, rir)
        assert got == scoring.select_rule(fe, st, clr, oor, req, rir), (trial, B, req, rir)


def test_support_states_can_be_clean_while_the_executed_trajectory_collides(oracle):
    """Pins why the dense check exists, on the oracle alone: the two WAM restart batches solved with Gauss-Newton have
    rows whose support-state collision cost is exactly 0 and whose up-sampled states penetrate an obstacle."""
    for p, J in ref.motivation_inputs():
        ro, so = oracle.robot(p.model), ref.oracle_sdf(oracle, p.sdf_origin, p.sdf_cell, p.sdf_data)
        res = oracle.batch_optimize(ro, so.handle, p.setting, p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
        sc = ref.oracle_score(oracle, p.model, ro, so, ref.delta_t(p.setting), J, res["traj"])
        cc = oracle.collision_cost(ro, so.handle, p.setting.total_step, res["traj"])
        np.testing.assert_allclose(sc["support_cost"], cc, rtol=0, atol=1e-12)
        clean = sc["support_cost"] == 0.0
        dirty = clean & (sc["dense_cost"] > 0.0)
        assert dirty.any(), (p.B, int(clean.sum()))
        assert (sc["min_clearance"][dirty] < 0.0).all()
        print(f"B={p.B} N={p.setting.total_step} inter_step={J}: {clean.sum()} support-clean rows, {dirty.sum()} of them "
              f"dense-dirty, worst clearance {sc['min_clearance'].min():.4f}, max |support - collision_cost| "
              f"{np.abs(sc['support_cost'] - cc).max():.2e}")
