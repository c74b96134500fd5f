"""The Pose2 maps of the kernels against the exact maps (tests/pose2_reference.py: mpmath, 60 digits, differenced
Jacobians), through the factor-level entry points, over the cases of tests/pose2_cases.py -- heading differences from
0 over 1e-18 to pi - 1e-9 in both signs, every switch of form at 0.99 and 1.01 times its value, four translations, four
first headings (two of them put c2.theta - c1.theta across the cut), two interpolation times, and a set in which the
interpolated tangent xi[2] lands in each band although the heading difference does not:

  * gp_prior_factor(5, lie=True): err and H1..H4 -- Log, its derivative, Ad of p1 and of the inverse of p2;
  * gp_interpolate(5, lie=True): conf and vel -- Exp of Log, compose, the heading wrap (compared on the circle);
  * obstacle_gp_factor of a Pose2 base with two spheres on the two ramp fields d = x and d = y, hinge on everywhere:
    H1..H4, and through them the interpolation Jacobians M1..M4 and the Exp derivative.

One call of each entry point holds all cases.  The oracle is a restatement of the same forms and cannot referee them;
the exact maps do.  The gate follows tests/test_gpu_step_backward_error.py: for every case and output
    e_gpu <= min(max(K * e_oracle, FLOOR), CAP),   e = max |got - exact| / scale   (tests/pose2_cases.py)
with e_oracle the oracle's error on the same case, computed here.  K and FLOOR come from one measured run
(profiles/pose2_maps_error.txt, written by scripts/pose2_maps_error.py, states the rule); CAP = 1e-12 is a condition:
double-precision prototypes of the cancellation-free forms reach 4e-15 at scale 1 (tests/test_pose2_reference_cpu.py)
and every defect of GTSAM's expressions exceeds it by 10 times or more wherever it exceeds 1e-11."""
from __future__ import annotations

import numpy as np
import pytest

import pose2_cases as pc

pytestmark = pytest.mark.gpu

CAP = pc.CAP
K = 32.0               # next power of two above 4 x 5.423, the largest e_gpu / e_oracle of the measured run (interp.vel)
FLOOR = 4 * 1.150e-15  # 4 x the largest e_gpu among the cases with e_oracle < 1e-16 of the measured run (interp.vel)


@pytest.fixture(scope="module")
def measured(engine, oracle):
    return pc.measure(engine, *pc.handles(engine)), pc.measure(oracle, *pc.handles(oracle))


@pytest.mark.parametrize("group", pc.GROUPS)
def test_gpu_maps_against_the_exact_maps(measured, group):
    e_gpu, e_orc = measured[0][group], measured[1][group]
    band = pc.case_bands(group)
    for k, (name, _, _) in enumerate(pc.BANDS):
        if (band == k).any():
            print(f"{group} {name}: e_gpu {e_gpu[band == k].max():.2e}  e_oracle {e_orc[band == k].max():.2e}")
    lim = np.minimum(np.maximum(K * e_orc, FLOOR), CAP)
    bad = np.flatnonzero(e_gpu > lim)
    worst = bad[np.argmax(e_gpu[bad])] if bad.size else -1
    assert bad.size == 0, (f"{group}: {bad.size} of {e_gpu.size} cases above the bound; the worst, case {worst} (band "
                           f"{pc.BANDS[band[worst]][0]}): e_gpu = {e_gpu[worst]:.3e}, e_oracle = {e_orc[worst]:.3e}")
