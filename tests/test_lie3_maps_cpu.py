"""The oracle's SO(3) / SE(3) maps against the exact maps (tests/lie3_reference.py), over the cases of
tests/lie3_cases.py: the workspace factor's error and Jacobian in orientation and in pose mode (Log on SO(3) and SE(3),
their derivatives, the link's body Jacobian) and the path check's deviations and costs (Exp of tau Log between two
targets, through tests/path_reference.py).

The oracle alone is held to CAP = 1e-12 here; the GPU is held to the oracle's own error on each case in
tests/test_gpu_lie3_maps.py.  With GTSAM 4.0's expressions, which the oracle carried before, this file fails: the
largest e per output was rot.err 6.3 (= 2 pi: next to pi the first-order branch takes its sign from a column of R, so
half the axes come out as their antipode; 6.2e-6 above that branch, 5.0e-12 from tr_3^2), rot.H 3.1 (7.4e-9 where
[w]x / 2 was dropped below theta^2 = 2.2e-16), pose.err 6.3 (4.4e-11 from the dropped w x T / 2), pose.H 3.1 (6.5e-10
from c2 next to 1e-5, whose small-angle constant has the wrong sign), path.rot_dev 2.2e-1 and path.cost 8.3e-2 (the
geodesic between two targets half a turn apart taken the other way round; path.pos_dev 8.6e-17 passes); a
float32-rounded target at pi - 1e-9 gave NaN (profiles/lie3_maps_error.txt has the table per band): seven tests of this
file fail there.  With the forms of csrc/lie_log.h the largest is 9.5e-16."""
from __future__ import annotations

import numpy as np
import pytest

import lie3_cases as lc


@pytest.fixture(scope="module")
def measured(oracle):
    h = lc.handles(oracle)
    e = lc.measure(oracle, h)
    e.update(lc.measure_path(oracle, h))
    return e


def test_case_list_is_the_one_the_issue_sets():
    cs = lc.cases()
    issue = [0.0, 1e-18, 3e-11, 9.9e-11, 1.01e-10, 1e-9, 1.4e-8, 1.6e-8, 1e-7, 1e-6, 9.9e-6, 1.01e-5, 1e-4, 3.1e-4, 3.2e-4,
             1e-3, 1e-2, 0.1, 1.0, 2.0, 3.0, np.pi - 1e-3, np.pi - 1e-4, np.pi - 2e-5, np.pi - 1.01e-5, np.pi - 9.9e-6,
             np.pi - 1e-6, np.pi - 1e-9]
    assert all(t in lc.THETAS for t in issue) and len(lc.THETAS) == len(issue) + 2 * len(lc.SWITCHES)
    for c in lc.SWITCHES:
        for f in (0.99, 1.01):
            assert any(abs(f * c - m) <= 1e-12 * c for m in lc.THETAS), (c, f)
    assert len(lc.AXES) == 8 and all(abs(np.linalg.norm(a) - 1.0) < 1e-15 for a in lc.AXES)
    assert min(abs(x) for x in lc.AXES[7] if x != 0.0) < 2e-8
    for mode in (lc.ORIENTATION, lc.POSE):
        mine = [c for c in cs if c[1] == mode]
        assert {c[3] for c in mine} == set(lc.THETAS)                       # every angle, in both modes
        for th in lc.THETAS:                                                # from 1 rad on about every axis, both signs
            if th >= 1.0:
                assert {c[4] for c in mine if c[3] == th} == set(range(8)), th
        assert {c[0] for c in mine} == {0, 1, 2}                            # every robot and configuration
        for g in (("rot" if mode == lc.ORIENTATION else "pose") + s for s in (".err", ".H")):
            assert set(lc.case_bands(g)) == set(range(len(lc.BANDS))), g    # a case in every band
    assert {c[5] for c in cs if c[1] == lc.POSE} == {0, 1, 2, 3}            # every translation
    assert 300 <= len(cs) <= 600
    assert sorted(sum(lc.PATH_CHUNKS, [])) == sorted(lc.THETAS) and lc.PATH_N <= 16 and len(lc.PATH_Q) <= 4
    assert [r for r in lc.PATH_RUNS] == [(1, lc.ORIENTATION), (3, lc.POSE)]
    lc.reference()         # asserts that no case is within 1e-12 of the cut


def test_link_jacobians_have_full_row_rank():
    import lie3_reference as ref
    for name, link, q in lc.CONFIGS[:2]:
        J = np.array(ref.fk(lc.models()[name].fk_model(), q, link)[1].tolist(), dtype=np.float64)
        assert J.shape == (6, 7) and np.linalg.svd(J, compute_uv=False)[-1] > 0.05


@pytest.mark.parametrize("group", lc.GROUPS)
def test_oracle_meets_the_cap(measured, group):
    e, band = measured[group], lc.case_bands(group)
    print(f"{group}: " + "  ".join(f"{lc.BANDS[k]} {e[band == k].max():.1e}" for k in range(len(lc.BANDS)) if (band == k).any()))
    worst = int(np.argmax(e))
    assert e[worst] <= lc.CAP, f"{group}: e = {e[worst]:.3e} at case {worst} (band {lc.BANDS[band[worst]]})"


def test_oracle_at_exactly_pi_on_the_group(oracle):
    """|omega| within 4 ulp of pi and Exp(omega) the nearest rotation of Rd^T Rm to CAP: at pi the two signs of omega
    are one rotation, so omega itself is not compared"""
    for (ulps, d), case in zip(lc.measure_pi(oracle, lc.handles(oracle)), lc.pi_cases()):
        print(f"mode {case[1]}: | |omega| - pi | = {ulps:.0f} ulp, max |Exp(omega) - Rrel| = {d:.2e}")
        assert ulps <= 4 and d <= lc.CAP


def test_oracle_stays_finite_on_targets_that_are_not_quite_rotations(oracle):
    for (ok, e_err, e_H), case in zip(lc.measure_nonortho(oracle, lc.handles(oracle)), lc.nonortho_cases()):
        print(f"mode {case[1]} theta {case[3]:.10g}: from the exact maps on the polar factor err {e_err:.1e} H {e_H:.1e}")
        assert ok
