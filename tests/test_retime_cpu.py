"""The re-timing rule (include/gpmp2mi.h "re-timing") without a GPU: gpmp2_amd/csrc/retime_rule.h, built by the host
compiler with -ffp-contract=off (tests/retime_shim.py), against the numpy statement of the same rule
(tests/retime_reference.py) on the seam of gpmp2mi_retime_path, and the properties the rule promises, on the numpy side
alone.

Bit for bit: the set ends K, x = sdot^2 (hence sdot: one correctly rounded square root), u, the stamps and the duration.
Both sides round every operation once and take exact minima and maxima, so no operation had to be excused and nothing
here is bounded in ulp.  `achieved` is four maxima of the same expressions and is compared exactly as well."""
import numpy as np
import pytest

import retime_reference as rr
import retime_shim

CASES = rr.path_cases()
MAX_RATE = 4.0


def path_of(c):
    qd, qL, qR, h = rr.path_from_traj(c["traj"], c["dt"], c["J"])
    return qd, qL, qR, rr.rate_caps(qd, c["vel"]), h


@pytest.fixture(scope="module")
def paths():
    return {name: path_of(c) for name, c in CASES}


def both(p, acc, **kw):
    qd, qL, qR, cap, h = p
    return rr.retime_path(qd, qL, qR, cap, acc, h, **kw), retime_shim.retime_path(qd, qL, qR, cap, acc, h, **kw)


def assert_same_bits(ref, got, what):
    assert got["status"] == ref["status"], what
    for name in ("K", "sdot", "u", "stamps", "achieved"):
        assert np.array_equal(got[name], ref[name], equal_nan=True), (what, name, got[name], ref[name])
    assert got["duration"] == ref["duration"], what


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_host_rule_gives_the_bits_of_the_numpy_rule(paths, name):
    c = dict(CASES)[name]
    rest = not c["traj"][0, c["traj"].shape[1] // 2:].any() and not c["traj"][-1, c["traj"].shape[1] // 2:].any()
    ends = [dict(), dict(max_rate=1.0), dict(rate_end=0.5), dict(rate_start=0.25, rate_end=0.25)]
    if rest:
        ends.append(dict(rate_start=0.0, rate_end=0.0))
    for kw in ends:
        kw = dict(dict(max_rate=MAX_RATE), **kw)
        ref, got = both(paths[name], c["acc"], **kw)
        assert_same_bits(ref, got, (name, kw))


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_reference_meets_every_limit_and_beats_the_uniform_stretch(paths, name):
    """a condition on the inputs, not a tolerance of the kernel: the numpy rule alone keeps velocity, acceleration at the
    ends of every stage and the cap within 1 + 1e-9; with free ends it is no slower than the uniform stretch, which is a
    feasible profile of these rows (the greedy pass is pointwise maximal); with max_rate = 1 it is never faster than
    planned"""
    c = dict(CASES)[name]
    qd, qL, qR, cap, h = paths[name]
    total = (c["traj"].shape[0] - 1) * c["dt"]
    r = rr.retime_path(qd, qL, qR, cap, c["acc"], h, max_rate=MAX_RATE, vel=c["vel"])
    assert r["status"] == rr.OK
    print(name, "achieved", r["achieved"], "duration", r["duration"], "of", total)
    assert r["achieved"][0] <= 1 + 1e-9 and r["achieved"][1] <= 1 + 1e-9 and r["achieved"][3] <= 1 + 1e-9
    assert (r["x"] >= r["K"][:, 0]).all() and (r["x"] <= r["K"][:, 1]).all()
    s = max(rr.uniform_scale(qd, qL, qR, c["vel"], c["acc"]), 1.0 / MAX_RATE)
    assert r["duration"] <= s * total * (1 + 1e-12), (r["duration"], s * total)
    one = rr.retime_path(qd, qL, qR, cap, c["acc"], h, max_rate=1.0, vel=c["vel"])
    assert one["status"] == rr.OK and (one["x"] <= 1.0).all()
    assert one["duration"] >= total * (1 - 1e-12)
    assert one["duration"] >= r["duration"]


def test_forced_zero_rates_are_feasible_for_rows_at_rest():
    n = 0
    for name, c in CASES:
        D = c["traj"].shape[1] // 2
        if c["traj"][0, D:].any() or c["traj"][-1, D:].any():
            continue
        ref, got = both(path_of(c), c["acc"], max_rate=MAX_RATE, rate_start=0.0, rate_end=0.0)
        assert ref["status"] == rr.OK and got["status"] == rr.OK, name
        assert ref["sdot"][0] == 0.0 and ref["sdot"][-1] == 0.0 and np.isfinite(ref["duration"])
        free = rr.retime_path(*path_of(c)[:4], c["acc"], path_of(c)[4], max_rate=MAX_RATE)
        assert ref["duration"] >= free["duration"]
        n += 1
    assert n >= 4


def test_a_forced_rate_above_the_cap_is_boundary():
    name, c = CASES[1]
    p = path_of(c)
    for kw in (dict(rate_start=MAX_RATE * 1.01), dict(rate_end=MAX_RATE * 1.01), dict(rate_start=3.9, max_rate=1.0)):
        kw = dict(dict(max_rate=MAX_RATE), **kw)
        ref, got = both(p, c["acc"], **kw)
        assert ref["status"] == rr.BOUNDARY and got["status"] == rr.BOUNDARY, kw
        assert got["duration"] == np.inf and np.isnan(got["sdot"]).all() and np.isnan(got["stamps"]).all()
        assert np.isnan(got["u"]).all() and np.isnan(got["achieved"]).all()


def test_a_pause_makes_every_b_zero_and_is_passed_at_the_rate_cap():
    """two equal support states at rest: q' = q'' = 0 over the whole interval, no row binds, x sits at max_rate^2"""
    name, c = CASES[0]
    D, J1 = c["traj"].shape[1] // 2, c["J"] + 1
    qd, qL, qR, cap, h = path_of(c)
    assert not qd[J1:2 * J1 + 1].any() and not qR[J1:2 * J1].any() and not qL[J1 + 1:2 * J1 + 1].any()
    ref, got = both((qd, qL, qR, cap, h), c["acc"], max_rate=MAX_RATE)
    assert ref["status"] == rr.OK
    assert_same_bits(ref, got, name)
    if J1 > 1:
        assert (ref["x"][J1 + 1:2 * J1] == MAX_RATE ** 2).all()


def test_non_finite_input_is_invalid_and_an_impossible_row_is_empty():
    name, c = CASES[2]
    qd, qL, qR, cap, h = path_of(c)
    for arr, k in ((qd, 1), (qL, 2), (qR, 0)):
        bad = arr.copy()
        bad[k, 0] = np.nan
        args = [bad if x is arr else x for x in (qd, qL, qR)]
        ref = rr.retime_path(*args, cap, c["acc"], h, max_rate=MAX_RATE)
        got = retime_shim.retime_path(*args, cap, c["acc"], h, max_rate=MAX_RATE)
        assert ref["status"] == rr.INVALID and got["status"] == rr.INVALID
        assert got["duration"] == np.inf and np.isnan(got["sdot"]).all()
    nocap = cap.copy()
    nocap[1] = np.nan
    assert retime_shim.retime_path(qd, qL, qR, nocap, c["acc"], h)["status"] == rr.INVALID
    # qdd_left of state 0 and qdd_right of the last state are not read
    qL2, qR2 = qL.copy(), qR.copy()
    qL2[0], qR2[-1] = np.nan, np.nan
    assert retime_shim.retime_path(qd, qL2, qR2, cap, c["acc"], h, max_rate=MAX_RATE)["status"] == rr.OK
    # a stage that no x can pass: at state 0 the path asks for an acceleration whatever the rate (q' = 0, q'' != 0 caps
    # x at acc / |q''|), and the forced end rate cannot be reached from there
    D = qd.shape[1]
    qd0, qR0 = np.zeros((2, D)), np.zeros((2, D))
    qL0 = np.zeros((2, D))
    qR0[0], qL0[1] = 4.0, 4.0
    ref = rr.retime_path(qd0, qL0, qR0, np.full(2, np.inf), np.full(D, 1.0), 0.01, max_rate=4.0, rate_end=3.0)
    got = retime_shim.retime_path(qd0, qL0, qR0, np.full(2, np.inf), np.full(D, 1.0), 0.01, max_rate=4.0, rate_end=3.0)
    assert ref["status"] == rr.EMPTY and got["status"] == rr.EMPTY


def test_results_do_not_depend_on_the_order_of_the_joints():
    """the set ends are exact extrema over the pairs: permuting the joints permutes rows and pairs and changes no bit"""
    name, c = CASES[3]
    qd, qL, qR, cap, h = path_of(c)
    D = qd.shape[1]
    perm = np.random.default_rng(1).permutation(D)
    a = retime_shim.retime_path(qd, qL, qR, cap, c["acc"], h, max_rate=MAX_RATE)
    b = retime_shim.retime_path(qd[:, perm], qL[:, perm], qR[:, perm], cap, c["acc"][perm], h, max_rate=MAX_RATE)
    for k in ("K", "sdot", "u", "stamps"):
        assert np.array_equal(a[k], b[k]), k
