"""The self-collision check (include/gpmp2mi.h "self-collision check") as far as the CPU oracle alone can say: the
restated definitions (tests/self_reference.py) agree with the SelfCollision factor, the gap the feature closes is there
(rows that pass the obstacle rule and collide with themselves), the list rule, the extended selection rule in numpy,
and that the inputs of tests/test_gpu_self.py decide their `worst` comparison."""
import numpy as np
import pytest

import score_reference as ref
import self_reference as sr
from gpmp2_amd import scoring
import gpmp2_amd as g


@pytest.fixture(scope="module")
def motivation(oracle):
    """the two WAM inputs of tests/score_reference.py solved by the oracle, with their obstacle and self scores"""
    out = []
    for p, J in ref.motivation_inputs():
        ro, so = oracle.robot(p.model), ref.oracle_sdf(oracle, p.sdf_origin, p.sdf_cell, p.sdf_data)
        res = oracle.batch_optimize(ro, so.handle, p.setting, p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
        dt = ref.delta_t(p.setting)
        table = sr.wam_table(oracle, p.model, ro)
        out.append(dict(p=p, J=J, ro=ro, res=res, dt=dt, table=table,
                        obstacle=ref.oracle_score(oracle, p.model, ro, so, dt, J, res["traj"]),
                        self=sr.oracle_self_score(oracle, p.model, ro, table, dt, J, res["traj"])))
    return out


def test_support_cost_is_the_sum_of_the_self_collision_factor_errors(oracle, motivation):
    arm3 = g.generateArm("SimpleThreeLinksArm")
    c5 = g.generateMobileArm("SimpleTwoLinksArm")
    m = motivation[0]
    wam_table = m["table"].copy()
    wam_table[:, 2] = 0.01
    folded = sr.line_traj([sr.FOLDED, sr.STRETCHED], 10)
    cases = [("arm3", arm3, sr.generated_table(oracle, arm3, oracle.robot(arm3), 2, None, 0.02), folded, sr.DELTA_T),
             ("wam", m["p"].model, wam_table, m["res"]["traj"], m["dt"]),
             ("config5", c5, sr.generated_table(oracle, c5, oracle.robot(c5), 2, None, 0.05), sr.case_traj("config5", 16),
              sr.DELTA_T)]
    for name, model, table, traj, dt in cases:
        ro = oracle.robot(model)
        D = model.dof()
        for J in (0, 3):
            sc = sr.oracle_self_score(oracle, model, ro, table, dt, J, traj)
            err, _ = oracle.self_collision_factor(ro, table, np.ascontiguousarray(traj[:, :, :D]).reshape(-1, D), jac=False)
            want = err.reshape(traj.shape[0], -1).sum(axis=1)
            print(f"{name} J={J}: support {sc['self_support_cost']}, max |d| {np.abs(sc['self_support_cost'] - want).max():.2e}")
            np.testing.assert_allclose(sc["self_support_cost"], want, rtol=1e-8, atol=1e-12, err_msg=name)
            assert want.max() > 0.0, (name, "no row of this input touches itself: the comparison shows nothing")
            if J == 0:
                assert np.array_equal(sc["self_dense_cost"], sc["self_support_cost"])
            else:
                assert (sc["self_dense_cost"] >= sc["self_support_cost"]).all()


def test_rows_that_pass_the_obstacle_rule_collide_with_themselves(motivation):
    """Pins why the check exists: of the rows the selection rule of "scoring" admits at required_clearance = 0, 9 of 15
    and 12 of 26 are in self-collision, by more than 5 cm at the worst."""
    expect = [(16, 15, 9), (32, 26, 12)]
    for m, (B, n_pass, n_hit) in zip(motivation, expect):
        assert m["table"].shape == (78, 4) and len(sr.candidate_pairs(m["p"].model, 2)) == 79
        res, ob, se = m["res"], m["obstacle"], m["self"]
        passing = scoring.eligible(res["final_error"], res["status"], ob["min_clearance"], ob["out_of_range"], 0.0, False)
        hit = passing & (se["min_self_clearance"] < 0.0)
        print(f"B={B}: {passing.sum()} rows pass the obstacle rule, {hit.sum()} of them touch themselves, worst overlap "
              f"{-se['min_self_clearance'].min():.4f} at row {se['min_self_clearance'].argmin()} "
              f"(state, pair) {se['worst'][se['min_self_clearance'].argmin()]}, min gap {np.nanmin(se['gap']):.2e}")
        assert (res["traj"].shape[0], int(passing.sum()), int(hit.sum())) == (B, n_pass, n_hit)
        assert se["min_self_clearance"].min() < -0.05
        assert (se["invalid"] == 0).all()
        # the row the old rule picks is clear of itself, so the extended rule picks it too -- out of fewer rows
        old = scoring.select_rule(res["final_error"], res["status"], ob["min_clearance"], ob["out_of_range"])
        new = scoring.select_rule(res["final_error"], res["status"], ob["min_clearance"], ob["out_of_range"], 0.0, False,
                                  se["min_self_clearance"], se["invalid"], 0.0)
        assert old == (1, n_pass) and new == (1, n_pass - n_hit)


def test_dense_states_come_closer_than_support_states(oracle, motivation):
    for m in motivation:
        sup = sr.oracle_self_score(oracle, m["p"].model, m["ro"], m["table"], m["dt"], 0, m["res"]["traj"])
        closer = sup["min_self_clearance"] - m["self"]["min_self_clearance"]
        assert (closer >= 0.0).all() and int((closer > 1e-3).sum()) == 2, closer


def test_the_list_rule(oracle):
    wam = g.generateArm("WAMArm")
    cand = sr.candidate_pairs(wam, 2)
    table = sr.generated_table(oracle, wam, oracle.robot(wam), 2, np.zeros((1, 7)))
    assert len(cand) == 79 and len(table) == 78
    assert (np.diff(cand[:, 0] * 100 + cand[:, 1]) > 0).all() and (cand[:, 0] < cand[:, 1]).all()   # lexicographic, A < B
    kept = {tuple(r) for r in table[:, :2].astype(int)}
    assert len([tuple(r) for r in cand if tuple(r) not in kept]) == 1
    # PR2: the tree, not the link index, and nothing that overlaps at the reference configuration
    pr2 = g.generateMobileArm("PR2")
    ro = oracle.robot(pr2)
    zero = np.zeros((1, 18))
    table = sr.generated_table(oracle, pr2, ro, 2, zero)
    centers, _ = oracle.sphere_centers(ro, zero)
    dist, te = sr.pair_clearance(pr2, centers, table[:, :2])
    assert len(table) > 1000 and not ((dist - te) < 0.0).any()
    link = np.array([s.link_id for s in pr2.spheres])
    by_index = {(a, b) for a in range(65) for b in range(a + 1, 65) if abs(link[a] - link[b]) >= 2}
    dist_i, te_i = sr.pair_clearance(pr2, centers, np.array(sorted(by_index)))
    assert int(((dist_i - te_i) < 0.0).sum()) == 13 and (dist_i - te_i).min() < -0.13    # why that rule is useless here
    by_tree = {tuple(r) for r in sr.candidate_pairs(pr2, 2)}
    assert by_tree != by_index
    # the first links of the two arms (2 and 9) hang off the torso: 2 joints apart, 7 by index; link 8 - link 9: 8 by tree
    par = sr.link_parents(pr2)
    assert sr.joint_distance(par, 2, 9) == 2 and sr.joint_distance(par, 8, 9) == 8 and sr.joint_distance(par, 0, 9) == 2
    # a fixed-base arm: the link-index difference; a point robot: no pair
    assert sr.joint_distance(sr.link_parents(wam), 1, 6) == 5
    assert len(sr.candidate_pairs(sr.models()["point2"](), 1)) == 0


INF, NAN = float("inf"), float("nan")


def _old_rule(fe, st, clr, oor, req, rir):
    """the rule of "scoring" as it stood before the self arguments, written out"""
    best, n = -1, 0
    for b in range(len(fe)):
        ok = np.isfinite(fe[b]) and (st is None or st[b] != 3) and clr[b] >= req and (not rir or oor is None or oor[b] == 0)
        if ok:
            n += 1
            if best < 0 or fe[b] < fe[best]:
                best = b
    return best, n


def test_select_rule_with_the_self_arguments():
    sel = scoring.select_rule
    ok = np.zeros(4, dtype=np.int32)
    fe, clr, oor = [3.0, 1.0, 2.0, 5.0], [0.1] * 4, [0] * 4
    # the cheapest row touches itself: skipped; at -inf taken again
    assert sel(fe, ok, clr, oor, min_self_clearance=[0.1, -0.01, 0.1, 0.1]) == (2, 3)
    assert sel(fe, ok, clr, oor, min_self_clearance=[0.1, -0.01, 0.1, 0.1], required_self_clearance=-INF) == (1, 4)
    assert sel(fe, ok, clr, oor, min_self_clearance=[0.1, 0.02, 0.1, 0.1], required_self_clearance=0.05) == (2, 3)
    # invalid > 0 is never eligible, whatever the clearance says; +inf (no valid pair, or an empty table) is clear
    assert sel(fe, ok, clr, oor, min_self_clearance=[0.1, INF, 0.1, 0.1], invalid=[0, 4, 0, 0], required_self_clearance=-INF) == (2, 3)
    assert sel(fe, ok, clr, oor, min_self_clearance=[INF] * 4, invalid=[0] * 4) == (1, 4)
    assert sel(fe, ok, clr, oor, min_self_clearance=[0.1, NAN, 0.1, 0.1], required_self_clearance=-INF) == (2, 3)
    assert sel(fe, ok, clr, oor, min_self_clearance=[-1.0] * 4) == (-1, 0)
    # ties still go to the lowest row
    assert sel([2.0, 1.0, 1.0, 1.0], ok, clr, oor, min_self_clearance=[0.1, -1.0, 0.1, 0.1]) == (2, 3)
    # the defaults reproduce the old answers
    rng = np.random.default_rng(1606)
    values = np.array([0.5, 1.0, 1.5, 2.0, 2.5, 3.0, NAN, INF])
    clears = np.array([-0.2, -0.05, 0.0, 0.03, 0.08, 0.3, INF, -INF, NAN])
    for trial in range(200):
        B = int(rng.integers(1, 60))
        fe = rng.choice(values, size=B)
        st = rng.integers(0, 5, size=B).astype(np.int32)
        clr = rng.choice(clears, size=B)
        oor = (rng.integers(0, 4, size=B) == 0).astype(np.int32)
        req, rir = float(rng.choice([0.0, 0.05, -0.1, -INF])), bool(rng.integers(0, 2))
        with np.errstate(invalid="ignore"):
            want = _old_rule(fe, st, clr, oor, req, rir)
        assert sel(fe, st, clr, oor, req, rir) == want, trial
        assert sel(fe, st, clr, oor, req, rir, np.full(B, INF), np.zeros(B, dtype=np.int32), 0.0) == want, trial
        mask = scoring.eligible(fe, st, clr, oor, req, rir)
        slf = rng.choice(clears, size=B)
        inv = (rng.integers(0, 5, size=B) == 0).astype(np.int32)
        with np.errstate(invalid="ignore"):
            both = mask & (slf >= 0.02) & (inv == 0)
        assert np.array_equal(scoring.eligible(fe, st, clr, oor, req, rir, slf, inv, 0.02), both), trial


def test_pair_tables_are_checked_in_python():
    assert scoring.pair_table([], 4).shape == (0, 4)
    assert np.array_equal(scoring.pair_table([[0, 2]], 4), [[0, 2, 0, 1]])
    for bad in ([[0, 4, 0, 1]], [[1, 1, 0, 1]], [[0.5, 1, 0, 1]], [[-1, 1, 0, 1]], [1, 2, 3, 4], [[0, 1, 0, 1, 5]]):
        with pytest.raises(ValueError):
            scoring.pair_table(bad, 4)


@pytest.mark.parametrize("case", sr.GPU_CASES, ids=[sr.case_id(c) for c in sr.GPU_CASES])
def test_the_gpu_inputs_decide_their_worst_comparison(oracle, case):
    """tests/test_gpu_self.py compares `worst` wherever the reference's runner-up is more than 1e-6 above its minimum and
    excuses at most 10 % of the rows; here the reference's own count of closer rows stays within that, input by input.
    The two-sphere point robot is the one exception by construction: its single distance is the same in every state, an
    exact tie (5, from dyadic coordinates at support states), which the tie rule decides -- asserted exactly there."""
    name, which, (N, J) = case
    model = sr.models()[name]()
    ro = oracle.robot(model)
    table = sr.case_table(name, which, oracle, model, ro)
    exp = sr.oracle_self_score(oracle, model, ro, table, sr.DELTA_T, J, sr.case_traj(name, N))
    B = len(exp["invalid"])
    print(f"{sr.case_id(case)}: P = {len(table)}, gaps {exp['gap']}, min clearance {exp['min_self_clearance']}")
    if name == "point2":
        assert (exp["gap"] == 0.0).all() and (exp["worst"] == 0).all() and (exp["min_self_clearance"] == 3.75).all()
        return
    assert sr.close_rows(exp) <= 0.1 * B
    assert (exp["invalid"] == 0).all()


def test_the_motivation_inputs_decide_their_worst_comparison(motivation):
    gaps = [float(np.nanmin(m["self"]["gap"])) for m in motivation]
    print("minimum gaps", gaps)
    for m in motivation:
        assert sr.close_rows(m["self"]) <= 0.1 * m["res"]["traj"].shape[0]


def test_folded_and_stretched_rows_have_the_signs_the_gpu_test_asserts(oracle):
    model = sr.models()["arm3s"]()
    ro = oracle.robot(model)
    for which, (N, J) in (("one", (1, 0)), (3, (9, 6)), ("generated", (16, 3)), ("all", (32, 3))):
        table = sr.case_table("arm3s", which, oracle, model, ro)
        exp = sr.oracle_self_score(oracle, model, ro, table, sr.DELTA_T, J, sr.case_traj("arm3s", N))
        assert exp["min_self_clearance"][0] < -0.05 and exp["self_dense_cost"][0] > 0.0      # folded: a certain overlap
        assert exp["min_self_clearance"][1] > 0.05 and exp["self_dense_cost"][1] == 0.0      # stretched: none
