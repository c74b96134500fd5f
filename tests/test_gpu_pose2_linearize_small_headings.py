"""The fused linearization of a Pose2 plan at heading steps inside the bands where GTSAM's expressions for the Pose2
maps lose digits (tests/pose2_cases.py): config 5 cut to N = 8 (handover_cases.pose2_n8), three trajectories -- every
heading step exactly 0 (what config 5 starts from: start heading == end heading), every step in 1e-5 .. 1e-3, and a
mix from 0 over 1e-18 up to 9.9e-3 -- without and with interpolated obstacle factors, so that lie_interpolate runs with
its Jacobians.  engine.linearize and graph_error against the oracle at the gate of
test_gpu_plan.test_config5_linearize_matches_oracle.  (The exact-value gate of the maps themselves is
tests/test_gpu_pose2_maps.py; here GPU and oracle must agree where, with the old forms, they differed by however cos
rounded next to a branch.)"""
from __future__ import annotations

import numpy as np
import pytest

import handover_cases

pytestmark = pytest.mark.gpu

STEPS = {
    "all zero": [0.0] * 8,
    "1e-5 .. 1e-3": [1.01e-5, -3e-5, 1e-4, -1e-3, 3e-5, -1.01e-5, 1e-3, -1e-4],
    "mixed": [0.0, 1e-18, 3e-11, 9.9e-11, -1.01e-10, 1e-8, 9.9e-6, -9.9e-3],
}


def _problem(inter):
    p = handover_cases.pose2_n8()
    p.setting.set_obs_check_inter(inter)
    B, N = len(STEPS), p.setting.total_step
    assert all(len(s) == N for s in STEPS.values())
    init = np.repeat(p.init, B, axis=0)
    for b, steps in enumerate(STEPS.values()):
        for i, w in enumerate(steps):
            init[b, i + 1, 2] = init[b, i, 2] + w
    p.init = init
    for name in ("start_conf", "start_vel", "end_conf", "end_vel"):
        setattr(p, name, np.repeat(getattr(p, name), B, axis=0))
    return p


@pytest.mark.parametrize("inter", [0, 2])
def test_pose2_linearize_small_headings(engine, oracle, inter):
    p = _problem(inter)
    th = p.init[:, :, 2]
    assert (np.diff(th[0]) == 0).all() and (np.abs(np.diff(th[1])) > 9e-6).all() and (np.abs(np.diff(th[1])) < 1.1e-3).all()
    args = (p.start_conf, p.start_vel, p.end_conf, p.end_vel)
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    ro, so = oracle.robot(p.model), oracle.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    a = engine.linearize(r, s, p.setting, *args, p.init)
    b = oracle.linearize(ro, so, p.setting, *args, p.init)
    for name, x, y in zip(("Hd", "Ho", "g"), a[:3], b[:3]):
        print(f"inter {inter} {name}: max |gpu - oracle| = {np.abs(x - y).max():.2e}, max |oracle| = {np.abs(y).max():.2e}")
    print(f"inter {inter} error: gpu {a[3]}, oracle {b[3]}")
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_allclose(x, y, atol=1e-9 * np.abs(y).max())
    np.testing.assert_allclose(a[3], b[3], rtol=1e-9)
    np.testing.assert_allclose(engine.graph_error(r, s, p.setting, *args, p.init),
                               oracle.graph_error(ro, so, p.setting, *args, p.init), rtol=1e-9)
