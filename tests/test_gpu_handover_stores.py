"""Moving or re-flavouring the stores that hand data from one kernel of a pass to the next changes no arithmetic, so
whole plans must return what they returned before, BIT FOR BIT: trajectory, iters, status and final_error of the plans
of tests/handover_cases.py against tests/golden/handover_stores.npz, recorded on an MI355X at the commit named inside
the fixture (scripts/record_handover_golden.py) -- the parent of the change that made k_assemble's stores of fac /
tiles / pend / coup write-through (tiles.h StorePolicy).  The raw tiles / fac / pend / coup buffers the last pass left
are compared through their SHA-256.

The shapes are the smallest at which the reordering can go wrong (handover_cases: the early return without a fused
level 2, level 2 as the top, a partly empty last group, the first level-4 and level-8 tasks, a trajectory that leaves in
pass 0), for Gauss-Newton, LM and Dogleg, plus one Pose2 plan and one 7-joint plan.  Parity with the oracle stays with
the existing tests."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

import handover_cases as hc

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "handover_stores.npz")
CASES = hc.cases()


@pytest.fixture(scope="module")
def recorded():
    with np.load(FIXTURE, allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    meta = json.loads(str(arrays.pop("meta")))
    assert len(meta["commit"]) == 40, meta["commit"]
    return arrays, meta


def test_fixture_covers_every_case(recorded):
    arrays, meta = recorded
    assert sorted(meta["raw"]) == sorted(CASES)
    assert sorted(arrays) == sorted(f"{c}/{k}" for c in CASES for k in hc.RESULT_KEYS)
    for c in CASES:
        if c.startswith("planar2"):     # one trajectory leaves in pass 0, the others iterate
            it = arrays[f"{c}/iters"]
            assert it[hc.ALREADY_OPTIMAL_ROW] == 0 and (it[: hc.ALREADY_OPTIMAL_ROW] >= 1).all(), (c, list(it))


@pytest.mark.parametrize("case", list(CASES))
def test_plan_returns_the_recorded_bits(engine, recorded, case):
    arrays, meta = recorded
    got = hc.run_case(engine, CASES[case])
    for k in ("iters", "status"):
        want = arrays[f"{case}/{k}"]
        assert np.array_equal(got[k], want), (case, k, list(got[k]), list(want), meta["commit"])
    for k in ("final_error", "traj"):
        want = arrays[f"{case}/{k}"]
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, (case, k)
        same = got[k].tobytes() == want.tobytes()
        assert same, (case, k, "max |diff|", float(np.abs(got[k] - want).max()), "recorded at", meta["commit"])
    assert got["raw"] == meta["raw"][case], (case, [n for n in got["raw"] if got["raw"][n] != meta["raw"][case][n]])


ASM_WT_MAX_B = 256      # cr_kernels.hip: plans of more trajectories keep plain hand-over stores in k_assemble


@pytest.mark.parametrize("opt", ["GN", "LM"])
def test_both_store_policies_return_the_same_bits(engine, opt):
    """The same problems through a plan of ASM_WT_MAX_B trajectories (write-through stores) and one of ASM_WT_MAX_B + 1
    (plain stores): every shared row agrees bit for bit.  (Gauss-Newton and LM plans choose every other form without
    looking at the number of trajectories: host/plan_create.hip choose_forms.)"""
    p = hc.planar2(8, opt)
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    res = {}
    for nb in (ASM_WT_MAX_B, ASM_WT_MAX_B + 1):
        idx = np.arange(nb) % hc.B
        pl = engine.plan(r, s, p.setting, nb)
        try:
            pl.set_problem(p.start_conf[idx], p.start_vel[idx], p.end_conf[idx], p.end_vel[idx], p.init[idx])
            pl.optimize()
            res[nb] = pl.result()
        finally:
            pl.close()
    a, b = res[ASM_WT_MAX_B], res[ASM_WT_MAX_B + 1]
    assert (a["iters"][: hc.ALREADY_OPTIMAL_ROW] >= 1).all(), list(a["iters"][: hc.B])
    for k in hc.RESULT_KEYS:
        assert a[k].tobytes() == b[k][:ASM_WT_MAX_B].tobytes(), (opt, k)
        assert b[k][ASM_WT_MAX_B].tobytes() == b[k][ASM_WT_MAX_B % hc.B].tobytes(), (opt, k)
