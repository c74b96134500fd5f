"""The optimizer's step control (no GPU): gpmp2_amd/csrc/step_control.h, the text the kernels call, built by the host
compiler (control_shim) and run against the CPU oracle on the 50 cases of the robot sweep, one trajectory at a time.

Outer loop: the oracle's error trace through first_decide / loop_decide must stop at the oracle's iteration with the
oracle's status.  Dogleg: every trial point of the oracle (its probe) through dogleg_blend / dogleg_iterate -- same
branch of the dogleg point, same band of the gain ratio, same retry decision, and the trust radius the next trial point
starts from.  LM: every tryLambda call of the oracle through lm_try_lambda -- same step_ok / stop and the next lambda.
The branches the sweep never reaches are table rows with the oracle line they restate.

Measured with this header against the oracle over the sweep (688 Dogleg rows, none within 1e-6 of a band edge, the
nearest 1.03e-3 away; 114 retries; Cauchy 104 / blend 248 / Newton 336; bands 493 / 57 / 24):
  largest relative difference of rho   1.99e-11  (q formed from the five scalars, the oracle's from the vectors)
  largest relative difference of Delta 5.74e-15  (3 |dx_d| from the scalars in the band rho >= 0.75)
The gates below are 100 times these, and never above 1e-9.  LM: 605 rows over the sweep's 14 LM cases (538 good steps,
61 bad steps, 6 stops), none within 1e-9 of a threshold; the sweep has no row with lin_change < 0 or a failed solve, so
those are table rows.  Outer loop: 174 GN, 78 Dogleg and 83 LM problems, all of the sweep."""
import math

import pytest

import control_shim as shim
from control_shim import MOVED, NOT_SPD, RETRY, RETURNED
from oracle import Oracle
from sweep_cases import robot_sweep_cases

RHO_RTOL = min(100 * 1.99e-11, 1e-9)
DELTA_RTOL = min(100 * 5.74e-15, 1e-9)
EDGE_GUARD, LM_GUARD, SKIP_CAP = 1e-6, 1e-9, 0.05
CONVERGED, MAX_ITER, ROLLED_BACK, NOT_SPD_STATUS, ALREADY_OPTIMAL = 0, 1, 2, 3, 4


@pytest.fixture(scope="module")
def sweep():
    """one record per trajectory of the sweep: the oracle's solve, its probe rows and the plan's rules"""
    orc = Oracle()
    out = []
    for case, name, opt, p in robot_sweep_cases(50):
        ro, so = orc.robot(p.model), orc.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
        rules = shim.rules_of(p.setting)
        for b in range(p.init.shape[0]):
            one = [a[b:b + 1] for a in (p.start_conf, p.start_vel, p.end_conf, p.end_vel)]
            with orc.dogleg_probe() as dl, orc.lm_probe() as lm:
                r = orc.batch_optimize(ro, so, p.setting, *one, p.init[b:b + 1], nthreads=1)
            assert len(dl.rows) < 256 and len(lm.rows) < 512      # the probes' capacity: no row was dropped
            out.append(dict(case=case, b=b, opt=opt, rules=rules, trace=r["error_trace"][0], iters=int(r["iters"][0]),
                            status=int(r["status"][0]), dl=dl.rows, lm=lm.rows))
    return out


def _lm_outcome(rules, row):
    """what iterate_lm (oracle_core.cpp:1529-1540) does after a tryLambda call with this probe row: flags, next lambda"""
    lam, step_ok, stop = row[0], bool(row[7]), bool(row[8])
    if step_ok:
        return RETURNED | MOVED, max(rules.lm_lower, lam / rules.lm_factor)
    if not stop:
        lam = lam * rules.lm_factor
        return (RETURNED if lam >= rules.lm_upper else 0), lam
    return RETURNED, lam


# ------------------------------------------------------------------------------- outer loop
def test_outer_loop_stops_where_the_oracle_stops(sweep):
    checked = {"GN": 0, "DOGLEG": 0, "LM": 0}
    for rec in sweep:
        if rec["status"] == NOT_SPD_STATUS:      # the trace alone does not say where it stopped
            continue
        rules, tr, tag = rec["rules"], rec["trace"], (rec["case"], rec["b"])
        act, status = shim.first_decide(rules, tr[0])
        it, prev = 0, tr[0]
        if rec["opt"] != "LM":
            while act == 0:
                it += 1
                act, status = shim.loop_decide(rules, it, True, prev, tr[it])
                if rec["opt"] == "GN":            # the fast path's single entry point is the same rule
                    assert shim.gn_decide(rules, it, prev, tr[it]) == (act, status), tag
                prev = tr[it]
        else:
            cur, rows = tr[0], list(rec["lm"])
            while act == 0:
                row = rows.pop(0)
                assert row[1] == cur, tag
                flags, _ = _lm_outcome(rules, row)
                if not flags & RETURNED:
                    continue
                counted = bool(flags & MOVED)
                it += counted
                cur = row[6] if counted else cur
                act, status = shim.loop_decide(rules, it, counted, prev, cur)
                prev = cur
            assert not rows, tag
        assert (it, status) == (rec["iters"], rec["status"]), (tag, it, status, rec["iters"], rec["status"])
        checked[rec["opt"]] += 1
    print("outer loop: problems checked", checked)
    assert min(checked.values()) >= 50


# ------------------------------------------------------------------------------- Dogleg
def _band(rho):
    return 0 if rho >= 0.75 else 1 if rho >= 0.25 else 2 if rho >= 0.0 else 3


def test_dogleg_rows_follow_the_oracle(sweep):
    rows = skipped = retries = 0
    branches, bands = [0, 0, 0], [0, 0, 0, 0]
    worst_rho = worst_delta = 0.0
    nearest_edge = math.inf
    for rec in sweep:
        if rec["opt"] != "DOGLEG":
            continue
        it = 0
        for k, row in enumerate(rec["dl"]):
            gg, gHg, gn, nn, uu, un, tau, Delta, rho, new_f = row
            tag = (rec["case"], rec["b"], k)
            cur_err = rec["trace"][it]
            rows += 1
            # the dogleg point: same branch as ComputeDoglegPoint (oracle_core.cpp:1591-1603)
            want = 0 if Delta * Delta < uu else 1 if tau != -1.0 else 2
            cu, cn, q = shim.dogleg_blend(gg, gHg, gn, nn, Delta)
            got = 0 if cn == 0.0 else 2 if (cu == 0.0 and cn == 1.0) else 1
            assert got == want, (tag, got, want)
            branches[want] += 1
            edge = min(abs(rho - e) for e in (0.0, 0.25, 0.75))
            nearest_edge = min(nearest_edge, edge)
            retry_row = rho < 0.0 and Delta > 1e-5
            if edge <= EDGE_GUARD:
                skipped += 1
            else:
                xnorm = math.sqrt(cu * cu * gg + 2.0 * cu * cn * gn + cn * cn * nn)
                flags, Delta_out = shim.dogleg_iterate(Delta, cur_err, new_f, q, xnorm)
                # the gain ratio the header forms (step_control.h: dogleg_iterate) next to the oracle's
                f_dec, m_dec = cur_err - new_f, cur_err - (cur_err + q)
                rho_h = 0.5 if (abs(f_dec) < 1e-15 or abs(m_dec) < 1e-15) else f_dec / m_dec
                d_rho = abs(rho_h - rho) / abs(rho)
                worst_rho = max(worst_rho, d_rho)
                band = _band(rho)
                bands[band] += 1
                assert _band(rho_h) == band, (tag, rho_h, rho)
                assert flags == ((RETURNED | MOVED) if band < 3 else RETRY if Delta > 1e-5 else RETURNED), (tag, flags, rho)
                if band == 1 or (band >= 2 and Delta > 1e-5):
                    assert Delta_out == (Delta if band == 1 else 0.5 * Delta), (tag, Delta_out, Delta)
                elif band == 0:
                    assert Delta_out == max(Delta, 3.0 * xnorm), tag
                if k + 1 < len(rec["dl"]):      # ... is the radius of the oracle's next trial point
                    nxt = rec["dl"][k + 1][7]
                    d_delta = abs(Delta_out - nxt) / nxt
                    worst_delta = max(worst_delta, d_delta)
                    assert d_delta <= DELTA_RTOL, (tag, Delta_out, nxt, d_delta)
                assert d_rho <= RHO_RTOL, (tag, rho_h, rho, d_rho)
            retries += retry_row
            if not retry_row:
                it += 1
        assert it == rec["iters"] or rec["status"] == NOT_SPD_STATUS, (rec["case"], rec["b"], it, rec["iters"])
    print(f"dogleg: rows {rows} skipped {skipped} retries {retries} branches {branches} bands {bands} "
          f"nearest edge {nearest_edge:.3g} worst rel rho {worst_rho:.3g} worst rel Delta {worst_delta:.3g}")
    assert rows >= 600 and skipped <= SKIP_CAP * rows
    assert min(branches) > 0 and min(bands[:3]) > 0 and retries > 0


# ------------------------------------------------------------------------------- LM
def _lm_near_threshold(rules, row):
    lam, err, solved, gd, dd, lin_change, new_err = row[:7]
    if not solved:
        return False
    scale = 0.5 * abs(gd) + 0.5 * lam * dd
    eps_lin = 2.220446049250313e-16 * err
    if abs(lin_change) <= LM_GUARD * scale or abs(lin_change - eps_lin) <= LM_GUARD * max(scale, eps_lin):
        return True
    if lin_change < 0:
        return False
    cost_change = err - new_err
    if lin_change > eps_lin:
        fid = cost_change / lin_change
        if abs(fid - rules.lm_min_fidelity) <= LM_GUARD * max(abs(fid), abs(rules.lm_min_fidelity)):
            return True
    min_abs = rules.rel_thresh * err
    return abs(abs(cost_change) - min_abs) <= LM_GUARD * min_abs


def test_lm_rows_follow_the_oracle(sweep):
    rows = skipped = 0
    seen = {"step_ok": 0, "bad step": 0, "stop": 0, "lin_change < 0": 0, "unsolved": 0}
    for rec in sweep:
        if rec["opt"] != "LM":
            continue
        rules = rec["rules"]
        for k, row in enumerate(rec["lm"]):
            tag = (rec["case"], rec["b"], k)
            rows += 1
            if _lm_near_threshold(rules, row):
                skipped += 1
                continue
            lam, err, solved, gd, dd, lin_change, new_err, step_ok, stop = row
            flags, lam_out = shim.lm_try_lambda(rules, lam, err, new_err, gd, dd, failed=not solved)
            want_flags, want_lam = _lm_outcome(rules, row)
            assert (flags, lam_out) == (want_flags, want_lam), (tag, flags, lam_out, want_flags, want_lam, list(row))
            if k + 1 < len(rec["lm"]):
                assert lam_out == rec["lm"][k + 1][0], tag
            seen["step_ok" if step_ok else "stop" if stop else "bad step"] += 1
            seen["lin_change < 0"] += bool(solved and lin_change < 0)
            seen["unsolved"] += not solved
    print(f"lm: rows {rows} skipped {skipped} seen {seen}")
    assert rows >= 100 and skipped <= SKIP_CAP * rows
    assert seen["step_ok"] > 0 and seen["bad step"] > 0


# ------------------------------------------------------------------------------- branches the sweep never reaches
def _rules(**kw):
    base = dict(opt_type=shim.OPT_GN, max_iter=10, no_increase=1, fixed_iters=0, rel_thresh=1e-2, abs_tol=1e-5, err_tol=1e-5,
                lm_lambda0=100.0, lm_factor=10.0, lm_upper=1e5, lm_lower=0.0, lm_min_fidelity=1e-3, dl_delta0=1.0)
    base.update(kw)
    return shim.StepRules(**base)


def test_table_dogleg():
    # oracle_core.cpp:1629-1637: rho < 0 and the radius already at its floor -> zero step, iterate() returns unmoved
    assert shim.dogleg_iterate(1e-5, 2.0, 3.0, -0.5, 1e-5) == (RETURNED, 1e-5)
    # :1629-1631 above the floor: halve and try again from the same linearization
    assert shim.dogleg_iterate(1e-3, 2.0, 3.0, -0.5, 1e-3) == (RETRY, 0.5 * 1e-3)
    # :1607-1609 rho = 0.5 when either difference is below 1e-15 -> middle band (:1623), radius kept
    assert shim.dogleg_iterate(0.3, 2.0, 2.0 - 1e-16, -0.5, 0.3) == (RETURNED | MOVED, 0.3)     # f_error - new_f
    assert shim.dogleg_iterate(0.3, 2.0, 1.0, -1e-16, 0.3) == (RETURNED | MOVED, 0.3)           # M_error - new_M
    # :1618-1621 rho >= 0.75 grows the radius to 3 |dx_d|; :1625-1626 0 <= rho < 0.25 halves it (not below the floor)
    assert shim.dogleg_iterate(0.3, 2.0, 1.0, -1.0, 0.25) == (RETURNED | MOVED, 0.75)
    assert shim.dogleg_iterate(0.3, 2.0, 1.9, -1.0, 0.25) == (RETURNED | MOVED, 0.5 * 0.3)
    assert shim.dogleg_iterate(1e-5, 2.0, 1.9, -1.0, 1e-5) == (RETURNED | MOVED, 1e-5)
    # :1563-1567 the Newton solve failed: not_spd, nothing else (optimize() :1686 returns the last values, status 3)
    assert shim.dogleg_iterate(0.3, 2.0, 1.0, -1.0, 0.25, failed=True) == (NOT_SPD, 0.3)


def test_table_gn():
    # oracle_core.cpp:1489-1493 failed solve -> not_spd; :1494-1498 otherwise always accept
    assert shim.gn_iterate(True) == NOT_SPD
    assert shim.gn_iterate(False) == RETURNED | MOVED


def test_table_lm():
    R = _rules(opt_type=shim.OPT_LM)
    # oracle_core.cpp:1535-1537 bad step at lambda * factor >= lm_upper: give up, iterate() returns unmoved
    assert shim.lm_try_lambda(R, 1e4, 2.0, 3.0, -1.0, 1e-6) == (RETURNED, 1e5)
    # ... below the limit: lambda grows, same linearization again
    assert shim.lm_try_lambda(R, 1e3, 2.0, 3.0, -1.0, 1e-6) == (0, 1e4)
    # :1525-1526, :1538-1539 |cost_change| < rel_thresh * error and the step is not good: stop, lambda kept
    assert shim.lm_try_lambda(R, 100.0, 2.0, 2.0 + 1e-3, -1.0, 1e-6) == (RETURNED, 100.0)
    # :1517 lin_change < 0 (g.delta > 0): neither step_ok nor stop -> lambda grows (:1535-1536)
    assert shim.lm_try_lambda(R, 100.0, 2.0, 1.0, 1.0, 0.0) == (0, 1000.0)
    # :1512-1513 the damped solve failed: the same
    assert shim.lm_try_lambda(R, 100.0, 2.0, 1.0, -1.0, 1e-6, failed=True) == (0, 1000.0)
    # :1529-1534 good step: accept, lambda / factor, not below lm_lower
    assert shim.lm_try_lambda(R, 100.0, 2.0, 1.0, -1.0, 1e-6) == (RETURNED | MOVED, 10.0)
    assert shim.lm_try_lambda(_rules(lm_lower=50.0), 100.0, 2.0, 1.0, -1.0, 1e-6) == (RETURNED | MOVED, 50.0)


def test_table_outer_loop():
    R = _rules()
    # oracle_core.cpp:1674 already optimal; :1675 max_iter <= 0; :1664-1671 a fixed-iteration round skips both exits
    assert shim.first_decide(R, 1e-6) == (1, ALREADY_OPTIMAL)
    assert shim.first_decide(_rules(max_iter=0), 1.0) == (1, MAX_ITER)
    assert shim.first_decide(R, 1.0)[0] == 0
    assert shim.first_decide(_rules(fixed_iters=3, max_iter=0), 1e-6)[0] == 0
    # :1688-1695 keep going / converged / out of iterations
    assert shim.loop_decide(R, 1, True, 2.0, 1.0)[0] == 0
    assert shim.loop_decide(R, 2, True, 1.0, 0.995) == (1, CONVERGED)
    assert shim.loop_decide(R, 10, True, 2.0, 1.0) == (1, MAX_ITER)
    # :1691-1693 the last step raised the error: rollback on (status 2, the values before) and off
    assert shim.loop_decide(R, 3, True, 1.0, 1.5) == (2, ROLLED_BACK)
    assert shim.loop_decide(_rules(no_increase=0), 3, True, 1.0, 1.5) == (1, CONVERGED)   # (abs_dec < 0 <= abs_tol)
    assert shim.loop_decide(R, 1, True, 1.0, 1.5) == (2, ROLLED_BACK)                     # converged at once, the same
    # an LM call that gave up leaves the error where it was: converged (abs_dec = 0), :1537 then :1688-1695
    assert shim.loop_decide(_rules(opt_type=shim.OPT_LM), 2, False, 1.0, 1.0) == (1, CONVERGED)
    # :1664-1671 fixed-iteration rounds: stop at the count whatever the errors say (status 1) ...
    F = _rules(fixed_iters=3)
    assert shim.loop_decide(F, 2, True, 1.0, 1.5)[0] == 0
    assert shim.loop_decide(F, 3, True, 1.0, 1.5) == (1, MAX_ITER)
    # ... and at an LM call that did not count: the oracle's remaining rounds would try from the same state with a
    # lambda at its limit and leave values, error and status (1) as they are
    assert shim.loop_decide(_rules(opt_type=shim.OPT_LM, fixed_iters=3), 1, False, 1.0, 1.0) == (1, MAX_ITER)
