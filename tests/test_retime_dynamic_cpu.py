"""The rule of "re-timing under torque limits" (include/gpmp2mi.h) without a GPU: gpmp2_amd/csrc/retime_affine_rule.h built
by the host compiler (tests/retime_affine_shim.py) against the numpy rule (tests/retime_dynamic_reference.py) bit for
bit, its degenerate forms against retime_rule.h, its statuses, and the properties of the re-timed rows of
torque_reference.GPU_CASES (48 rows) with coefficients from torque_reference.inverse_dynamics."""
import numpy as np
import pytest

import retime_affine_shim as shim
import retime_dynamic_reference as dr
import retime_reference as rr
import retime_shim
import torque_reference as tq

PATH_CASES = rr.path_cases()
MAX_RATE = 4.0
PROFILE = ("K", "sdot", "u", "stamps", "duration", "status", "achieved")


def _bits(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a.view(np.int64)


def _same(a, b, names=PROFILE, what=""):
    for k in names:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k, a[k], b[k])


def _path(c):
    qd, qL, qR, h = rr.path_from_traj(c["traj"], c["dt"], c["J"])
    return qd, qL, qR, rr.rate_caps(qd, c["vel"]), h


def _extra_counts(D):
    return sorted({0, 1, min(D, 8), 8})


@pytest.mark.parametrize("name", [n for n, _ in PATH_CASES])
def test_host_rule_has_the_bits_of_the_numpy_rule(name):
    c = dict(PATH_CASES)[name]
    qd, qL, qR, cap, h = _path(c)
    Md, D = qd.shape
    seen, signs = set(), set()
    for R in _extra_counts(D):
        rng = np.random.default_rng(1000 * R + Md)
        rows = dr.random_affine(rng, Md, R)
        signs.update(np.sign(rows[2]).reshape(-1).tolist())
        for kw in (dict(), dict(rate_end=0.125), dict(rate_start=0.25, rate_end=0.25), dict(rate_start=MAX_RATE * 1.01)):
            kw = dict(dict(max_rate=MAX_RATE), **kw)
            host = shim.retime_affine(qd, qL, qR, cap, c["acc"], *rows, h, **kw)
            ref = dr.retime_affine(qd, qL, qR, cap, c["acc"], *rows, h, **kw)
            _same(host, ref, what=(name, R, kw))
            seen.add(host["status"])
            if host["status"] == dr.OK and R:
                assert host["achieved"][4] <= 1 + 1e-9, (name, R, kw, host["achieved"])
                assert 0 < host["achieved"][5] < 1
    assert dr.OK in seen
    assert signs >= {-1.0, 0.0, 1.0}          # both signs of cu, and rows that cap x


@pytest.mark.parametrize("name", [n for n, _ in PATH_CASES])
def test_no_affine_row_or_no_bound_is_the_rule_of_retime_rule_h(name):
    c = dict(PATH_CASES)[name]
    qd, qL, qR, cap, h = _path(c)
    Md = qd.shape[0]
    for kw in (dict(), dict(rate_end=0.125), dict(rate_start=MAX_RATE * 1.01)):
        kw = dict(dict(max_rate=MAX_RATE), **kw)
        plain = retime_shim.retime_path(qd, qL, qR, cap, c["acc"], h, **kw)
        plain["achieved"] = np.concatenate([plain["achieved"], plain["achieved"][:2] * 0])     # [4], [5]: 0, or NaN
        empty = np.zeros((Md, 0))
        _same(shim.retime_affine(qd, qL, qR, cap, c["acc"], empty, empty, empty, empty, np.zeros(0), h, **kw), plain,
              what=(name, "R = 0", kw))
        rows = list(dr.random_affine(np.random.default_rng(7), Md, 3))
        rows[4] = np.full(3, np.inf)
        rows[3][2, 1] = np.nan                     # a row without a bound is not looked at
        _same(shim.retime_affine(qd, qL, qR, cap, c["acc"], *rows, h, **kw), plain, what=(name, "no bound", kw))


def test_a_row_without_offset_is_the_two_sided_row():
    rng = np.random.default_rng(11)
    for cx, cu, A in zip(rng.normal(size=400), rng.normal(size=400), rng.uniform(0.1, 9.0, 400)):
        for a, b in ((cx, cu), (cx, 0.0), (0.0, 0.0), (cx, -0.0), (-0.0, cu)):
            for off in (0.0, -0.0):
                assert np.array_equal(_bits(shim.row_affine(a, b, off, A)), _bits(shim.row(a, b, A))), (a, b, off, A)
    assert np.array_equal(shim.row_affine(1.0, 2.0, 0.5, np.inf), [-np.inf, np.inf, 0.0, np.inf])


def test_both_signs_of_cu_and_a_row_that_caps_x():
    # |2 x + 4 u + 1| <= 3: -1 - x/2 <= u <= 1/2 - x/2
    assert np.array_equal(shim.row_affine(2.0, 4.0, 1.0, 3.0), [-1.0, 0.5, -0.5, np.inf])
    # |2 x - 4 u + 1| <= 3: -1/2 + x/2 <= u <= 1 + x/2
    assert np.array_equal(shim.row_affine(2.0, -4.0, 1.0, 3.0), [-0.5, 1.0, 0.5, np.inf])
    # cu == 0: |2 x + 1| <= 3 caps x at 1, |-2 x + 1| <= 3 at 2, and neither bounds u
    assert np.array_equal(shim.row_affine(2.0, 0.0, 1.0, 3.0), [-np.inf, np.inf, 0.0, 1.0])
    assert np.array_equal(shim.row_affine(-2.0, 0.0, 1.0, 3.0), [-np.inf, np.inf, 0.0, 2.0])
    assert np.array_equal(shim.row_affine(0.0, 0.0, 1.0, 3.0), [-np.inf, np.inf, 0.0, np.inf])
    # in the pass: one row with cu == 0 everywhere holds x at its cap
    Md = 6
    qd, z = np.full((Md, 1), 1.0), np.zeros((Md, 1))
    out = shim.retime_affine(qd, z, z, np.full(Md, np.inf), None, z + 2.0, z + 2.0, z, z + 1.0, [3.0], 0.1, max_rate=4.0)
    assert out["status"] == dr.OK and np.array_equal(out["sdot"], np.ones(Md)) and out["achieved"][4] == 1.0
    assert out["achieved"][5] == 1.0 / 3.0


def test_static_and_invalid_rows():
    c = dict(PATH_CASES)["long-D3N20J4"]
    qd, qL, qR, cap, h = _path(c)
    Md = qd.shape[0]
    rng = np.random.default_rng(2)
    for R in (1, 8):
        rows = dr.random_affine(rng, Md, R, static=True)               # |off| == bound at one state
        for f in (shim.retime_affine, dr.retime_affine):
            out = f(qd, qL, qR, cap, c["acc"], *rows, h, max_rate=MAX_RATE, rate_start=MAX_RATE * 1.01)
            assert out["status"] == dr.STATIC                          # ahead of BOUNDARY
            assert np.isinf(out["duration"]) and np.isnan(out["sdot"]).all() and np.isnan(out["achieved"]).all()
        ok = dr.random_affine(rng, Md, R)
        assert shim.retime_affine(qd, qL, qR, cap, c["acc"], *ok, h, max_rate=MAX_RATE)["status"] == dr.OK
        for which in range(4):
            for value in (np.nan, np.inf):
                bad = [x.copy() for x in ok]
                bad[which][Md // 2, 0] = value
                bad[3][1, 0] = bad[4][0]                                   # and static elsewhere: INVALID goes first
                for f in (shim.retime_affine, dr.retime_affine):
                    assert f(qd, qL, qR, cap, c["acc"], *bad, h, max_rate=MAX_RATE)["status"] == dr.INVALID
        edge = [x.copy() for x in ok]                                  # the two entries that are never read
        edge[0][0, 0] = np.nan
        edge[1][-1, 0] = np.nan
        _same(shim.retime_affine(qd, qL, qR, cap, c["acc"], *edge, h, max_rate=MAX_RATE),
              shim.retime_affine(qd, qL, qR, cap, c["acc"], *ok, h, max_rate=MAX_RATE))


# ------------------------------------------------------------------------------------- the 48 rows of the torque cases
VEL = 3.0


@pytest.fixture(scope="module")
def made(oracle):
    return {name: (tq.models()[name](), tq.case_table(name)) for name in ("one", "two", "wam", "arm8")}


def dynamic_rows(oracle, made, case, coef=None):
    """the numpy rule on every row of a case, and the uniform stretch of each: [(result, stretch)]"""
    name, (N, J), B = case
    model, table = made[name]
    D, dt = model.dof(), tq.case_dt(N)
    traj = tq.case_traj(name, N, B)
    coef = dr.coefficients(oracle, model, table, dt, J, traj) if coef is None else coef
    score = tq.reference_torque_score(oracle, model, table, dt, J, traj)
    out = []
    for b in range(B):
        r = dr.retime_dynamic_traj(traj[b], coef[b], dr.torque_limits(table, D), dt, J, vel=np.full(D, VEL),
                                   max_rate=MAX_RATE)
        qd = rr.path_from_traj(traj[b], dt, J)[0]
        out.append((r, dr.uniform_stretch(score["torque_time_scale"][b], qd, np.full(D, VEL))))
    return out


def test_properties_of_the_re_timed_torque_cases(oracle, made):
    shorter = longer = 0
    for case in tq.GPU_CASES:
        T = tq.DURATION
        for b, (r, stretch) in enumerate(dynamic_rows(oracle, made, case)):
            what = (tq.case_id(case), b)
            assert r["status"] == dr.OK, what
            assert r["achieved"][4] <= 1 + 2.0 ** -50, (what, r["achieved"][4] - 1)
            assert r["achieved"][5] < 1, what
            assert r["duration"] <= max(stretch, 1.0 / MAX_RATE) * T * (1 + 1e-12), (what, r["duration"], stretch * T)
            if stretch > 1.0 / MAX_RATE:
                longer += 1
                shorter += r["duration"] < stretch * T
    print("rows whose uniform stretch exceeds T / max_rate:", longer, "of which strictly shorter:", shorter)
    assert longer > 0 and 2 * shorter >= longer, (shorter, longer)


def test_host_rule_has_the_bits_of_the_numpy_rule_on_a_torque_case(oracle, made):
    case = ("arm8", (8, 7), 3)
    name, (N, J), B = case
    model, table = made[name]
    dt, traj = tq.case_dt(N), tq.case_traj(name, N, B)
    coef = dr.coefficients(oracle, model, table, dt, J, traj)
    for b in range(B):
        qd, qL, qR, h = rr.path_from_traj(traj[b], dt, J)
        cap = rr.rate_caps(qd, np.full(8, VEL))
        c = coef[b]
        args = (qd, qL, qR, cap, None, c[:, 1], c[:, 2], c[:, 0], c[:, 3], table["torque"], h)
        _same(shim.retime_affine(*args, max_rate=MAX_RATE), dr.retime_affine(*args, max_rate=MAX_RATE), what=b)


def test_p_is_the_mass_matrix_times_the_path_derivative_on_the_planar_two_link(oracle, made):
    model, table = made["two"]
    N, J = 9, 6
    dt, traj = tq.case_dt(N), tq.case_traj("two", N, 3)
    U = oracle.interpolate_traj(2, False, None, dt, J, traj)
    q, v = U[:, :, :2].reshape(-1, 2), U[:, :, 2:].reshape(-1, 2)
    free = dict(table, gravity=np.zeros(3))
    want = tq.planar_two_link(free, q, np.zeros_like(q), v).reshape(3, -1, 2)          # M(q) q': no velocity, no gravity
    coef = dr.coefficients(oracle, model, table, dt, J, traj)
    assert tq.err(coef[:, :, 0], want).max() < 1e-13
    hold = tq.planar_two_link(table, q, np.zeros_like(q), np.zeros_like(q)).reshape(3, -1, 2)
    assert tq.err(coef[:, :, 3], hold).max() < 1e-13
    # the rows of the rule are the torque: tau = p u + m x + tau_g at x = 1, u = 0 is the torque at planned timing
    score = tq.reference_torque_score(oracle, model, table, dt, J, traj)
    assert tq.err(coef[:, :, 2] + coef[:, :, 3], score["tau"]).max() < 1e-13
