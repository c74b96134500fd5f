"""k_linearize_arm's tail -- who adds the last two partial records, who stores which 16-byte piece of a chunk's records,
which wavefront evaluates the GP prior and when -- changes no arithmetic, so one linearization and whole plans must
return what they returned before, BIT FOR BIT: the plans of tests/linearize_tail_cases.py against
tests/golden/linearize_tail.npz, recorded on an MI355X at the commit named inside the fixture
(scripts/record_linearize_tail_golden.py) -- the parent of the change that made the record store cooperative.

Per case: g and err of gpmp2mi_plan_linearize as values, Hdiag and Hoff through their SHA-256; trajectory, iters, status
and final_error of an optimize and the SHA-256 of the raw tiles / fac / pend / coup buffers its last pass left
(handover_cases.run_case); for two cases the same of a fixed-iteration plan (gpmp2mi_plan_update)."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

import handover_cases as hc
import linearize_tail_cases as lc

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linearize_tail.npz")
CASES = lc.cases()


@pytest.fixture(scope="module")
def recorded():
    with np.load(FIXTURE, allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    meta = json.loads(str(arrays.pop("meta")))
    assert len(meta["commit"]) == 40, meta["commit"]
    return arrays, meta


def _same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), (what, "max |diff|", float(np.abs(got - want).max()))


def _same_results(got, arrays, prefix, raw, what):
    for k in ("iters", "status"):
        want = arrays[f"{prefix}/{k}"]
        assert np.array_equal(got[k], want), (what, k, list(got[k]), list(want))
    for k in ("final_error", "traj"):
        _same_bits(got[k], arrays[f"{prefix}/{k}"], (what, k))
    assert got["raw"] == raw, (what, [n for n in got["raw"] if got["raw"][n] != raw[n]])


def test_fixture_covers_every_case(recorded):
    arrays, meta = recorded
    assert sorted(meta["raw"]) == sorted(meta["lin_digest"]) == sorted(CASES)
    assert sorted(meta["update_raw"]) == sorted(lc.UPDATE_CASES)
    want = [f"{c}/{k}" for c in CASES for k in lc.RESULT_KEYS + lc.LIN_VALUE_KEYS]
    want += [f"{c}/update/{k}" for c in lc.UPDATE_CASES for k in lc.RESULT_KEYS]
    assert sorted(arrays) == sorted(want)
    for c in CASES:      # the last trajectory leaves in pass 0, the others iterate
        it, err = arrays[f"{c}/iters"], arrays[f"{c}/lin_err"]
        assert it[lc.ALREADY_OPTIMAL_ROW] == 0 and (it[: lc.ALREADY_OPTIMAL_ROW] >= 1).all(), (c, list(it))
        assert err[lc.ALREADY_OPTIMAL_ROW] == 0.0 and (err[: lc.ALREADY_OPTIMAL_ROW] > 0.0).all(), (c, list(err))


@pytest.mark.parametrize("case", list(CASES))
def test_linearization_returns_the_recorded_bits(engine, recorded, case):
    arrays, meta = recorded
    got = lc.run_linearize(engine, CASES[case])
    for k in lc.LIN_VALUE_KEYS:
        _same_bits(got[k], arrays[f"{case}/{k}"], (case, k, "recorded at", meta["commit"]))
    want = meta["lin_digest"][case]
    assert got["lin_digest"] == want, (case, [n for n in want if got["lin_digest"][n] != want[n]])


@pytest.mark.parametrize("case", list(CASES))
def test_plan_returns_the_recorded_bits(engine, recorded, case):
    arrays, meta = recorded
    _same_results(hc.run_case(engine, CASES[case]), arrays, case, meta["raw"][case], (case, "recorded at", meta["commit"]))


@pytest.mark.parametrize("case", list(lc.UPDATE_CASES))
def test_fixed_iteration_plan_returns_the_recorded_bits(engine, recorded, case):
    arrays, meta = recorded
    _same_results(lc.run_update(engine, CASES[case]), arrays, f"{case}/update", meta["update_raw"][case],
                  (case, "update", "recorded at", meta["commit"]))
