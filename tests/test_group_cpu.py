"""The leader rule of "distinct alternatives" (include/gpmp2mi.h) on the host: gpmp2mi_group_rows against the literal
loop of tests/group_reference.py and against gpmp2_amd.scoring.group_rule, on random symmetric matrices and on the cases
that separate the rule from a plausible wrong one."""
import numpy as np
import pytest

import group_reference as gr
from gpmp2_amd import engine as E
from gpmp2_amd import scoring

INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def _all_three(eng, dist, score, eligible, radius):
    """library, numpy rule and reference agree; returns the library's answer"""
    dist = np.asarray(dist, dtype=np.float64)
    lib = eng.group_rows(dist, score, eligible, radius)
    ref = gr.rule(dist, np.asarray(score, dtype=np.float64), eligible, radius)
    own = scoring.group_rule(dist, score, eligible, radius)
    for name, r, o in zip(("mode", "leaders", "sizes"), ref, own):
        assert np.array_equal(lib[name], r), (name, lib[name], r)
        assert np.array_equal(o, r), (name, o, r)
    assert lib["n_modes"] == ref[3] == own[3]
    return lib


def _sym(rows):
    d = np.array(rows, dtype=np.float64)
    assert np.array_equal(d, d.T, equal_nan=True)
    return d


CHAIN = _sym([[0.0, 1.0, 2.0], [1.0, 0.0, 1.0], [2.0, 1.0, 0.0]])   # a-b and b-c within 1.5, a-c not


def test_a_chain_tells_the_leader_rule_from_single_linkage(eng):
    got = _all_three(eng, CHAIN, [2.0, 1.0, 3.0], None, 1.5)          # b ranked first: one mode of three
    assert got["n_modes"] == 1 and list(got["mode"]) == [0, 0, 0] and list(got["leaders"]) == [1, -1, -1]
    assert list(got["sizes"]) == [3, 0, 0]
    got = _all_three(eng, CHAIN, [1.0, 2.0, 3.0], None, 1.5)          # a ranked first: {a, b} and {c}
    assert got["n_modes"] == 2 and list(got["mode"]) == [0, 0, 1] and list(got["leaders"]) == [0, 2, -1]
    assert list(got["sizes"]) == [2, 1, 0]
    got = _all_three(eng, CHAIN, [3.0, 2.0, 1.0], None, 1.5)          # c ranked first: {c, b} and {a}
    assert list(got["mode"]) == [1, 0, 0] and list(got["leaders"]) == [2, 0, -1]


def test_score_ties_go_to_the_lowest_row(eng):
    got = _all_three(eng, CHAIN, [1.0, 1.0, 1.0], None, 1.5)
    assert list(got["leaders"]) == [0, 2, -1] and list(got["mode"]) == [0, 0, 1]
    got = _all_three(eng, CHAIN, [2.0, 1.0, 1.0], None, 0.5)
    assert list(got["leaders"]) == [1, 2, 0] and list(got["mode"]) == [2, 0, 1]


def test_ineligible_and_non_finite_rows_do_not_take_part(eng):
    d = np.zeros((5, 5))
    got = _all_three(eng, d, [NAN, 0.5, -INF, 1.0, INF], [1, 0, 1, 1, 1], 1.0)
    assert list(got["mode"]) == [-1, -1, -1, 0, -1] and got["n_modes"] == 1
    assert list(got["leaders"]) == [3, -1, -1, -1, -1] and list(got["sizes"]) == [1, 0, 0, 0, 0]
    got = _all_three(eng, d, [1.0] * 5, [0] * 5, 1.0)
    assert got["n_modes"] == 0 and (got["mode"] == -1).all() and (got["leaders"] == -1).all() and (got["sizes"] == 0).all()
    got = _all_three(eng, d, [3.0, 2.0, 1.0, 5.0, 4.0], [1, 2, -1, 0, 7], 1.0)     # any non-zero int is eligible
    assert list(got["mode"]) == [0, 0, 0, -1, 0] and list(got["leaders"])[:2] == [2, -1]


def test_a_row_of_nan_distances_leads_a_mode_of_its_own(eng):
    d = np.zeros((4, 4))
    d[2, :] = d[:, 2] = NAN
    got = _all_three(eng, d, [1.0, 2.0, 3.0, 4.0], None, INF)
    assert list(got["mode"]) == [0, 0, 1, 0] and list(got["leaders"]) == [0, 2, -1, -1] and list(got["sizes"]) == [3, 1, 0, 0]
    got = _all_three(eng, d, [4.0, 3.0, 1.0, 2.0], None, 1.0)          # also when it is ranked first
    assert list(got["mode"]) == [1, 1, 0, 1] and list(got["leaders"]) == [2, 3, -1, -1]


def test_radius_zero_and_infinity(eng):
    d = _sym([[0.0, 0.0, 1e-300, 1.0], [0.0, 0.0, 1e-300, 1.0], [1e-300, 1e-300, 0.0, 1.0], [1.0, 1.0, 1.0, 0.0]])
    got = _all_three(eng, d, [1.0, 2.0, 3.0, 4.0], None, 0.0)          # only exact zeros join
    assert list(got["mode"]) == [0, 0, 1, 2] and got["n_modes"] == 3
    got = _all_three(eng, d, [1.0, 2.0, 3.0, 4.0], None, INF)
    assert list(got["mode"]) == [0, 0, 0, 0] and got["n_modes"] == 1 and list(got["sizes"]) == [4, 0, 0, 0]
    d[0, 3] = d[3, 0] = INF                                            # inf <= inf
    assert _all_three(eng, d, [1.0, 2.0, 3.0, 4.0], None, INF)["n_modes"] == 1


def test_no_rows_and_one_row(eng):
    got = _all_three(eng, np.zeros((0, 0)), np.zeros(0), None, 1.0)
    assert got["n_modes"] == 0 and got["mode"].size == 0
    got = _all_three(eng, [[0.0]], [3.0], None, 0.0)
    assert got["n_modes"] == 1 and list(got["mode"]) == [0] and list(got["leaders"]) == [0] and list(got["sizes"]) == [1]
    got = _all_three(eng, [[NAN]], [3.0], None, 0.0)                   # a leader is a member of its own mode
    assert got["n_modes"] == 1 and list(got["mode"]) == [0] and list(got["sizes"]) == [1]
    got = _all_three(eng, [[0.0]], [NAN], None, 0.0)
    assert got["n_modes"] == 0 and list(got["mode"]) == [-1]


def test_random_symmetric_matrices_and_the_first_leader_is_the_selection(eng):
    rng = np.random.default_rng(20261)
    for trial in range(120):
        B = int(rng.integers(1, 90))
        pts = rng.standard_normal((B, 2)) * rng.choice([0.3, 1.0, 3.0])
        d = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(axis=2))
        d = np.maximum(d, d.T)
        if trial % 3 == 0:                                # a few NaN / inf pairs, kept symmetric
            for _ in range(3):
                a, b = rng.integers(0, B, size=2)
                d[a, b] = d[b, a] = rng.choice([NAN, INF])
        score, eligible = gr.scores_with_ties(rng, B)
        radius = float(rng.choice([0.0, 0.2, 0.7, 1.5, INF]))
        got = _all_three(eng, d, score, eligible if trial % 4 else None, radius)
        el = eligible if trial % 4 else np.ones(B, dtype=np.int32)
        # leaders[0] is the row the selection rule of "scoring" picks: eligibility as a clearance of +-1
        best, n = scoring.select_rule(score, None, np.where(el != 0, 1.0, -1.0), None)
        assert int(got["leaders"][0]) == best if B else True, (trial, got["leaders"][:3], best)
        assert int(got["sizes"].sum()) == n == int((got["mode"] >= 0).sum())
        # every output may be NULL
        lib, sc = eng.lib, np.ascontiguousarray(score)
        only_n = E.C.c_int(-1)
        assert lib.gpmp2mi_group_rows(B, E.dptr(d), E.dptr(sc), None if not trial % 4 else E.iptr(eligible), radius, None,
                                      None, None, E.C.byref(only_n)) == 0
        assert only_n.value == got["n_modes"]
    assert eng.lib.gpmp2mi_group_rows(2, E.dptr(np.zeros((2, 2))), E.dptr(np.zeros(2)), None, 1.0, None, None, None, None) == 0
