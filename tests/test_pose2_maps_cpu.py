"""The oracle's Pose2 maps against the exact maps (tests/pose2_reference.py), over the cases of tests/pose2_cases.py:
the GP prior's error and Jacobians (Log, its derivative, Ad), the interpolated state and velocity (Exp of Log, compose,
the heading wrap) and the obstacle factor's Jacobians on two ramp fields (the Exp derivative).

The oracle alone is held to CAP = 1e-12 here; the GPU is held to the oracle's own error on each case in
tests/test_gpu_pose2_maps.py.  With GTSAM's expressions, which the oracle carried before, this file fails: the largest
e per output was prior.err 5.2e-7, prior.H1 / H3 4.9e-2, interp.conf 2.6e-7, interp.vel 1.6e-6, obs.H1 / H3 2.2e-2,
obs.H2 2.1e-7, obs.H4 1.2e-7 (profiles/pose2_maps_error.txt has the table per band); with the cancellation-free forms
the largest is 6.7e-15."""
from __future__ import annotations

import numpy as np
import pytest

import pose2_cases as pc


@pytest.fixture(scope="module")
def measured(oracle):
    return pc.measure(oracle, *pc.handles(oracle))


def test_case_list_is_the_one_the_issue_sets():
    cs = pc.cases()
    assert len(pc.W_VALUES) == 2 * (len(pc.W_MAGNITUDES) - 1) + 1 and 0.0 in pc.W_VALUES
    for c in pc.SWITCHES:
        for f in (0.99, 1.01):
            assert any(abs(f * c - m) <= 1e-12 * c for m in pc.W_MAGNITUDES), (c, f)
    assert len(cs["prior"][0]) == len(pc.W_VALUES) * len(pc.TRANSLATIONS) * len(pc.HEADINGS)
    assert len(cs["interp"][0]) >= 2 * len(cs["prior"][0])
    # the heading difference of the inputs crosses the cut for the two headings next to it
    c1, _, c2 = cs["prior"][:3]
    assert (np.abs(c2[:, 2] - c1[:, 2]) > np.pi).sum() >= 20
    # xi[2] lands in every band at w = 1
    xi = np.abs(np.array(pc.reference()["xi"])[np.asarray(cs["interp"][5]) == pc.XI_W])
    for lo, hi in ((0.0, 1e-10), (1e-10, 1e-5), (1e-5, 1e-2), (1e-2, 0.1)):
        assert ((xi >= lo) & (xi < hi)).any(), (lo, hi)


@pytest.mark.parametrize("group", pc.GROUPS)
def test_oracle_meets_the_cap(measured, group):
    e, band = measured[group], pc.case_bands(group)
    print(f"{group}: " + "  ".join(f"{pc.BANDS[k][0]} {e[band == k].max():.1e}" for k in range(len(pc.BANDS))
                                 if (band == k).any()))
    worst = int(np.argmax(e))
    assert e[worst] <= pc.CAP, f"{group}: e = {e[worst]:.3e} at case {worst} (band {pc.BANDS[band[worst]][0]})"


def test_oracle_interpolation_jacobians_meet_the_cap(oracle):
    """M1..M4 of the interpolated state themselves, in the state's own chart (the obstacle groups above see them through
    the sphere Jacobians): every 64th interpolation case and every 16th of the steered-tangent set"""
    import pose2_reference as ref
    cs = pc.cases()["interp"]
    M = len(cs[0])
    pick = sorted(set(range(0, M, 64)) | set(np.flatnonzero(np.asarray(cs[5]) == pc.XI_W)[::16].tolist()))
    worst = 0.0
    for m in pick:
        c1, v1, c2, v2, tau = (x[m] for x in cs[:5])
        got = oracle.gp_interpolate_jac(pc.DOF, True, np.eye(pc.DOF), pc.DT, float(tau), c1, v1, c2, v2)
        want = ref.interpolate_jacobians(ref.gp_coef(pc.DT, tau), *(ref.M(x) for x in (c1, v1, c2, v2)))
        scale = max(1.0, float(np.abs(np.concatenate([c1, v1, c2, v2])).max()))
        e = max(pc._err(got[k][0], want[k]) for k in range(4)) / scale
        worst = max(worst, e)
        assert e <= pc.CAP, (m, e)
    print(f"M1..M4 of {len(pick)} cases: largest e {worst:.2e}")
