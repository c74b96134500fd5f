"""The selection rules of gpmp2_amd/scoring.py against each other and against their documented conditions, on random rows
with planted ties, NaN, +-inf and not-SPD rows.  Pure numpy."""
import numpy as np
import pytest

from gpmp2_amd import scoring

B = 16
SPECIAL = (np.nan, np.inf, -np.inf)


def rows(seed):
    rng = np.random.default_rng(seed)

    def floats(lo, hi):
        x = rng.uniform(lo, hi, B)
        x[rng.choice(B, 3, replace=False)] = SPECIAL
        return x

    fe = np.round(floats(0.0, 4.0), 0)                      # few distinct values: ties among the minima
    r = dict(final_error=fe, status=rng.choice([0, 1, 2, 3, 4], B), min_clearance=floats(-0.1, 0.3),
             out_of_range=rng.choice([0, 0, 0, 1], B), min_self_clearance=floats(-0.1, 0.3),
             invalid=rng.choice([0, 0, 0, 2], B), pos_margin=floats(-0.1, 0.3), motion_invalid=rng.choice([0, 0, 0, 1], B),
             time_scale=np.abs(floats(0.5, 1.5)), torque_time_scale=np.abs(floats(0.5, 1.5)),
             torque_invalid=rng.choice([0, 0, 0, 1], B), min_moving_clearance=floats(-0.1, 0.3),
             moving_invalid=rng.choice([0, 0, 0, 1], B), max_pos_dev=floats(0.0, 0.2), max_rot_dev=floats(0.0, 0.2),
             path_invalid=rng.choice([0, 0, 0, 1], B), retime_status=rng.choice([0, 0, 0, 1, 2, 3], B),
             duration=floats(0.5, 3.0))
    t = dict(required_clearance=0.05, require_in_range=bool(seed % 2), required_self_clearance=0.02,
             required_pos_margin=0.01, max_time_scale=float(rng.choice([0.0, 1.0, 1.2, np.inf])),
             required_moving_clearance=0.03, max_pos_dev_allowed=0.1, max_rot_dev_allowed=0.15,
             max_duration=float(rng.choice([1.5, 2.5, np.inf])))
    return r, t


def lowest_minimiser(fe, ok):
    """the documented pick, written without argmin: the first row among the eligible whose final_error no other
    eligible row undercuts"""
    idx = [b for b in range(len(fe)) if ok[b]]
    for b in idx:
        if all(fe[b] <= fe[c] for c in idx):
            return b, len(idx)
    return -1, 0


def base_mask(r, t, self_check=True):
    ok = np.isfinite(r["final_error"]) & (r["status"] != 3)
    with np.errstate(invalid="ignore"):
        ok &= r["min_clearance"] >= t["required_clearance"]
        if t["require_in_range"]:
            ok &= r["out_of_range"] == 0
        if self_check:
            ok &= (r["min_self_clearance"] >= t["required_self_clearance"]) & (r["invalid"] == 0)
    return ok


def motion_mask(r, t):
    with np.errstate(invalid="ignore"):
        return base_mask(r, t) & (r["motion_invalid"] == 0) & (r["pos_margin"] >= t["required_pos_margin"])


BASE = ("final_error", "status", "min_clearance", "out_of_range")
SELF = ("min_self_clearance", "invalid")


def args(r, t, rkeys, tkeys):
    return dict({k: r[k] for k in rkeys}, **{k: t[k] for k in tkeys})


@pytest.mark.parametrize("seed", range(50))
def test_rules_agree_with_each_other_and_with_their_conditions(seed):
    r, t = rows(seed)
    bt, st = ("required_clearance", "require_in_range"), ("required_self_clearance",)
    plain = args(r, t, BASE, bt)
    checked = args(r, t, BASE + SELF, bt + st)
    # without their own inputs the extended rules are select_rule
    for a in (plain, checked):
        want = scoring.select_rule(**a)
        assert scoring.feasible_rule(**a) == want and scoring.moving_rule(**a) == want
        assert scoring.dynamic_rule(**a) == want
    assert scoring.path_rule(**plain) == scoring.select_rule(**plain)
    assert scoring.select_rule(**plain) == lowest_minimiser(r["final_error"], base_mask(r, t, False))
    assert scoring.select_rule(**checked) == lowest_minimiser(r["final_error"], base_mask(r, t))
    # dynamic_rule without torque inputs is feasible_rule
    feas = args(r, t, BASE + SELF + ("pos_margin", "time_scale", "motion_invalid"), bt + st + ("required_pos_margin", "max_time_scale"))
    assert scoring.dynamic_rule(**feas) == scoring.feasible_rule(**feas)
    with np.errstate(invalid="ignore"):
        assert scoring.feasible_rule(**feas) == lowest_minimiser(
            r["final_error"], motion_mask(r, t) & (r["time_scale"] <= t["max_time_scale"]))
        dyn = dict(feas, torque_time_scale=r["torque_time_scale"], torque_invalid=r["torque_invalid"])
        scale = np.maximum(np.maximum(0.0, r["time_scale"]), r["torque_time_scale"])
        assert scoring.dynamic_rule(**dyn) == lowest_minimiser(
            r["final_error"], motion_mask(r, t) & (r["torque_invalid"] == 0) & (scale <= t["max_time_scale"]))
        # the scale test holds even without a scale: the floor 0 against max_time_scale
        no_scale = {k: v for k, v in feas.items() if k != "time_scale"}
        assert scoring.dynamic_rule(**no_scale) == lowest_minimiser(
            r["final_error"], motion_mask(r, t) & (0.0 <= t["max_time_scale"]))
    # retimed_rule with every row OK and no duration bound is feasible_rule without time_scale
    no_ts = {k: v for k, v in feas.items() if k not in ("time_scale", "max_time_scale")}
    all_ok = np.full(B, scoring.RETIME_OK)
    assert scoring.retimed_rule(retime_status=all_ok, duration=np.ones(B), max_duration=np.inf, **no_ts) == \
        scoring.feasible_rule(**no_ts)
    with np.errstate(invalid="ignore"):
        assert scoring.retimed_rule(retime_status=r["retime_status"], duration=r["duration"],
                                    max_duration=t["max_duration"], **no_ts) == lowest_minimiser(
            r["final_error"], motion_mask(r, t) & (r["retime_status"] == 0) & (r["duration"] <= t["max_duration"]))
        mov = dict(checked, min_moving_clearance=r["min_moving_clearance"], moving_invalid=r["moving_invalid"],
                   required_moving_clearance=t["required_moving_clearance"])
        assert scoring.moving_rule(**mov) == lowest_minimiser(
            r["final_error"], base_mask(r, t) & (r["moving_invalid"] == 0)
            & (r["min_moving_clearance"] >= t["required_moving_clearance"]))
        pth = dict(plain, max_pos_dev=r["max_pos_dev"], max_rot_dev=r["max_rot_dev"], path_invalid=r["path_invalid"],
                   max_pos_dev_allowed=t["max_pos_dev_allowed"], max_rot_dev_allowed=t["max_rot_dev_allowed"])
        assert scoring.path_rule(**pth) == lowest_minimiser(
            r["final_error"], base_mask(r, t, False) & (r["path_invalid"] == 0)
            & (r["max_pos_dev"] <= t["max_pos_dev_allowed"]) & (r["max_rot_dev"] <= t["max_rot_dev_allowed"]))


def test_no_eligible_row_is_minus_one():
    fe = np.full(B, np.nan)
    z, i = np.zeros(B), np.zeros(B, dtype=np.int32)
    for rule in (scoring.select_rule, scoring.feasible_rule, scoring.dynamic_rule, scoring.moving_rule, scoring.path_rule):
        assert rule(fe, i, z, i) == (-1, 0)
    assert scoring.retimed_rule(fe, i, z, i, retime_status=i, duration=z) == (-1, 0)
