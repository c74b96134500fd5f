"""The heads of the Gauss-Newton pass kernels take their sizes from the kernel arguments and request a trajectory's
words in one batch; the pass-closing kernels count arrivals and continuing trajectories in one word.  Neither changes
any arithmetic, so the runs of tests/pass_heads_cases.py must return what they returned before, BIT FOR BIT: trajectory,
final error, error trace (up to each trajectory's last iteration), iterations and status against
tests/golden/pass_heads.npz, recorded on an MI355X at the commit named inside the fixture
(scripts/record_pass_heads_golden.py).

A wrong published count ends a run early or adds passes, so the Gauss-Newton cases also pin the launch counts their
timing reports: the step kernel runs max(iters) + 1 times -- the pass in which the last trajectory stops is the last --
and the linearization once more, because the driver enqueues it ahead of the count.  The one exception is the driver's
own: a run that reaches its pass cap (max(iters) equals the iteration cap: max_iter, or the fixed iterations of an update
round) ends on the cap and enqueues no linearization ahead of it."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

import pass_heads_cases as pc

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pass_heads.npz")
CASES = pc.cases()


@pytest.fixture(scope="module")
def recorded():
    with np.load(FIXTURE, allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    meta = json.loads(str(arrays.pop("meta")))
    assert len(meta["commit"]) == 40, meta["commit"]
    return arrays, meta


def test_fixture_covers_every_case(recorded):
    arrays, meta = recorded
    assert sorted(meta["launches"]) == sorted(CASES)
    assert sorted(arrays) == sorted(f"{c}/{k}" for c in CASES for k in pc.RESULT_KEYS)
    # what makes the cases the cases they claim to be
    it = arrays["planar2_N8_GN/iters"]
    assert it[-1] == 0 and (it[:-1] >= 1).all(), list(it)                    # one leaves in pass 0, the others iterate
    assert list(arrays["planar2_N8_GN_maxiter1/iters"]) == [1, 1, 0]
    assert (arrays["planar2_N8_GN_update/iters"] == pc.UPDATE_ITERS).all()
    assert arrays["planar2_N8_GN_B257/iters"].shape == (pc.BIG_B,)
    assert arrays["queue_5_through_2_GN/iters"].shape == (pc.QUEUE_M,)
    assert set(pc.GN_LAUNCH_CASES) <= set(CASES)


@pytest.mark.parametrize("case", list(CASES))
def test_run_returns_the_recorded_bits(engine, recorded, case):
    arrays, meta = recorded
    got = CASES[case](engine)
    for k in ("iters", "status"):
        want = arrays[f"{case}/{k}"]
        assert np.array_equal(got[k], want), (case, k, list(got[k][:8]), list(want[:8]), meta["commit"])
    for k in ("final_error", "trace", "traj"):
        want = arrays[f"{case}/{k}"]
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, (case, k)
        same = got[k].tobytes() == want.tobytes()
        assert same, (case, k, "max |diff|", float(np.nanmax(np.abs(got[k] - want))), "recorded at", meta["commit"])
    print(f"{case}: launches {got['launches']}, recorded {meta['launches'][case]}")
    assert got["launches"] == meta["launches"][case], (case, got["launches"], meta["launches"][case])
    if case in pc.GN_LAUNCH_CASES:
        top, cap = int(got["iters"].max()), pc.GN_LAUNCH_CASES[case]
        assert top <= cap, (case, top, cap)
        steps, lins = got["launches"]["gn_step_cr"], got["launches"]["linearize"]
        assert steps == top + 1, (case, steps, top)
        assert lins == steps + (0 if top == cap else 1), (case, lins, steps, top, cap)
