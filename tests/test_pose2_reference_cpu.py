"""Pins tests/pose2_reference.py, the exact Pose2 reference of the map tests: round trips to 1e-40, the differenced
derivative against the closed-form inverse right Jacobian at O(1) angles, and planted slips in a double-precision
prototype of the maps, each of which the reference must report above the cap of the map tests (and the unslipped
prototype below it)."""
from __future__ import annotations

import math

import numpy as np
import pytest

import pose2_cases as pc
import pose2_reference as ref
from pose2_reference import mp, mpf

ROUND_TRIP = mpf(10) ** -40


def test_exp_and_log_are_inverse_to_1e_40():
    for w in pc.W_VALUES:
        for t in pc.TRANSLATIONS:
            v = ref.M(t + (w,))
            back = ref.Log(ref.Exp(v))
            assert max(abs(a - b) for a, b in zip(back, v)) <= ROUND_TRIP, (w, t)
            p = ref.M(t + (w,))
            again = ref.Exp(ref.Log(p))
            assert max(abs(a - b) for a, b in zip(again, p)) <= ROUND_TRIP * max(1, abs(t[0])), (w, t)


def test_log_takes_the_principal_heading():
    for th, want in ((4.0, 4.0 - 2 * mp.pi), (-4.0, 2 * mp.pi - 4.0), (7.0, 7.0 - 2 * mp.pi)):
        assert abs(ref.Log(ref.M((0.3, 0.2, th)))[2] - want) <= ROUND_TRIP
    assert ref.principal(+mp.pi) == +mp.pi and abs(ref.principal(-mp.pi) - mp.pi) <= ROUND_TRIP      # (-pi, pi]
    assert ref.Exp(ref.M((0.3, -0.2, 0.0))) == ref.M((0.3, -0.2, 0.0))          # the w == 0 limit is exact
    assert ref.Log(ref.M((0.3, -0.2, 0.0))) == ref.M((0.3, -0.2, 0.0))


def test_group_identities():
    a, b = ref.M((0.4, -1.1, 2.9)), ref.M((-3.0, 0.6, -2.5))
    e = ref.compose(a, ref.inverse(a))
    assert max(abs(e[0]), abs(e[1]), abs(ref.principal(e[2]))) <= ROUND_TRIP
    back = ref.compose(a, ref.between(a, b))
    assert max(abs(back[0] - b[0]), abs(back[1] - b[1]), abs(ref.circular(back[2], b[2]))) <= ROUND_TRIP
    d = ref.M((0.1, -0.2, 0.3, 0.4))
    x = ref.M((0.4, -1.1, 2.9, 0.7))
    assert max(abs(p - q) for p, q in zip(ref.local(x, ref.retract(x, d)), d)) <= ROUND_TRIP


def _closed_form_dlog(p):
    """the inverse right Jacobian of SE(2) at v = Log(p), textbook form in mpf (good at O(1) angles at 60 digits)"""
    v = ref.Log(p)
    w = v[2]
    hc = mp.sin(w) / (2 * (1 - mp.cos(w)))
    return [[w * hc, -w / 2, v[0] / w - v[0] * hc + v[1] / 2],
            [w / 2, w * hc, v[1] / w - v[0] / 2 - v[1] * hc],
            [0, 0, 1]]


@pytest.mark.parametrize("w", [0.3, -1.0, 2.0, 3.0, -3.1])
def test_differenced_derivative_is_the_closed_form(w):
    p = ref.M((0.7, -0.4, w))
    J = ref.difference(lambda x: ref.Log(x), (p,), ("state",))[0]
    want = _closed_form_dlog(p)
    worst = max(abs(J[r][c] - want[r][c]) for r in range(3) for c in range(3))
    print(f"w = {w}: differenced - closed form = {float(worst):.1e}")
    # 60 digits: rounding u |Log| / STEP = 1e-60 * 4 / 1e-25 a term, a few terms; truncation STEP^2 = 1e-50
    assert worst <= mpf(10) ** -33


# ------------------------------------------------------------------------------------------------ planted slips
def _proto_log(p, slip=None):
    a = 0.5 * p[2]
    h = 1.0 if a == 0.0 else a * math.cos(a) / math.sin(a)
    ay = 0.0 if slip == "dropped w/2 y" else a * p[1]
    return [h * p[0] + ay, -a * p[0] + h * p[1], p[2]]


def _proto_dlog(p, slip=None):
    v, w = _proto_log(p), p[2]
    if slip == "first order at 5e-6":
        return [[1, 0, 0.5 * v[1]], [0, 1, -0.5 * v[0]], [0, 0, 1]]
    a = 0.5 * w
    h = 1.0 if a == 0.0 else a * math.cos(a) / math.sin(a)
    if slip == "hc through 1 - cos":
        hc = 0.5 * math.sin(w) / (1 - math.cos(w))
        return [[w * hc, -a, v[0] / w - v[0] * hc + 0.5 * v[1]], [a, w * hc, v[1] / w - 0.5 * v[0] - v[1] * hc],
                [0, 0, 1]]
    w2 = w * w
    g = (w * (1 / 12 + w2 * (1 / 720 + w2 * (1 / 30240 + w2 / 1209600))) if abs(w) < 1e-2
         else 1 / w - 0.5 * math.cos(a) / math.sin(a))
    return [[h, -a, v[0] * g + 0.5 * v[1]], [a, h, v[1] * g - 0.5 * v[0]], [0, 0, 1]]


def _proto_H1(p1, p2, slip=None):
    """-Hlog Ad(p2^-1) Ad(p1) of the GP prior, in doubles"""
    def ad(p):
        c, s = math.cos(p[2]), math.sin(p[2])
        y = -p[1] if slip == "sign in Ad" else p[1]
        return np.array([[c, -s, y], [s, c, -p[0]], [0, 0, 1]])

    def inv(p):
        c, s = math.cos(p[2]), math.sin(p[2])
        return [-(c * p[0] + s * p[1]), -(-s * p[0] + c * p[1]), -p[2]]

    i1 = inv(p1)
    c, s = math.cos(i1[2]), math.sin(i1[2])
    bt = [i1[0] + c * p2[0] - s * p2[1], i1[1] + s * p2[0] + c * p2[1], math.atan2(math.sin(p2[2] - p1[2]),
                                                                                   math.cos(p2[2] - p1[2]))]
    return -np.array(_proto_dlog(bt)) @ ad(inv(p2)) @ ad(p1), bt


def _second(p1, t, w):
    p2 = ref.compose(ref.M(p1), ref.M(t + (w,)))
    return [float(p2[0]), float(p2[1]), float(p2[2])]


def _measure_proto(w, slip):
    """e of the prototype's Log, its derivative and the prior's H1 at heading step w, translation (0.7, -0.4)"""
    p1 = [0.5, -0.25, 0.0]
    p2 = _second(p1, (0.7, -0.4), w)
    H1, bt = _proto_H1(p1, p2, slip)
    x1, x2 = ref.M(p1), ref.M(p2)
    z = ref.M((0.0, 0.0, 0.0))
    r_H = ref.gp_prior_jacobians(pc.DT, x1, z, x2, z)
    e_H1 = pc._err(H1, [row[:3] for row in r_H[0][:3]])
    btm = ref.M(bt)
    e_log = pc._err(_proto_log(bt, slip), ref.Log(btm))
    e_dlog = pc._err(_proto_dlog(bt, slip), ref.difference(lambda x: ref.Log(x), (btm,), ("state",))[0])
    return max(e_log, e_dlog, e_H1)      # scale 1: every input is below 1


SLIPS = [("dropped w/2 y", 1e-8), ("first order at 5e-6", 5e-6), ("hc through 1 - cos", 1.01e-5), ("sign in Ad", 1e-4),
         ("hc through 1 - cos", 1e-3)]


@pytest.mark.parametrize("slip,w", SLIPS, ids=[f"{s.replace(' ', '_')}_at_{w:g}" for s, w in SLIPS])
def test_planted_slip_is_reported_above_the_cap(slip, w):
    clean, slipped = _measure_proto(w, None), _measure_proto(w, slip)
    print(f"{slip} at w = {w:g}: e = {slipped:.2e}, the prototype without it {clean:.2e}, cap {pc.CAP:.0e}")
    assert clean <= pc.CAP / 100, "the cancellation-free prototype itself must sit far below the cap"
    assert slipped > 10 * pc.CAP


def test_prototype_meets_the_cap_at_every_heading_step():
    """the double-precision prototype of the forms in csrc/device_math.h, over the whole case list: <= 1e-14 at scale 1"""
    worst = max(_measure_proto(w, None) for w in pc.W_VALUES)
    print(f"worst e of the prototype over {len(pc.W_VALUES)} heading steps: {worst:.2e}")
    assert worst <= 1e-14
