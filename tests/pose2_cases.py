"""The cases of the Pose2 map tests: shared by tests/test_pose2_maps_cpu.py, tests/test_gpu_pose2_maps.py and
scripts/pose2_maps_error.py, which all measure through `measure` below.

A case is a pair of support states (c1, v1, c2, v2) of dof 5 = Pose2 x R^2 (the obstacle factor uses the pose part,
dof 3): the second pose is the first composed with (translation, heading difference w), rounded to doubles; everything
is then measured from those doubles.  Heading differences run through every band of the old and the new forms, both
signs; translations through O(1), zero, large and small; the first heading through 0, pi/2 and two values next to the
cut, so that c2.theta - c1.theta crosses +-pi.

For every case and output group, e = max |got - reference| / scale with
scale = max(1, largest |input coordinate or velocity| of the case, largest |field value| used).
"""
from __future__ import annotations

import functools
import math

import numpy as np

import pose2_reference as ref
from pose2_reference import mp, mpf

PI = math.pi
# every constant at which the code under test switches form (csrc/device_math.h POSE2_SERIES_BELOW; the exact zero of
# sin(a) / a needs no neighbours): each enters at 0.99 and 1.01 times its value
SWITCHES = [1e-2]
W_MAGNITUDES = [0.0, 1e-18, 3e-11, 9.9e-11, 1.01e-10, 1e-9, 1e-8, 1e-7, 1e-6, 9.9e-6, 1.01e-5, 3e-5, 1e-4, 1e-3, 9.9e-3,
                1.01e-2, 0.1, 1.0, 3.0, PI - 1e-6, PI - 1e-9]
for _c in SWITCHES:
    for _f in (0.99, 1.01):
        if not any(abs(_f * _c - m) <= 1e-12 * _c for m in W_MAGNITUDES):
            W_MAGNITUDES.append(_f * _c)
W_VALUES = [0.0] + [s * m for m in W_MAGNITUDES if m != 0.0 for s in (1.0, -1.0)]
TRANSLATIONS = [(0.7, -0.4), (0.0, 0.0), (30.0, -20.0), (1e-3, 2e-3)]
HEADINGS = [0.0, PI / 2, 3.0, -3.1]
TAU_FRACTIONS = [1.0 / 3.0, 1.0 / 2.0]
# the tangent xi[2] = l12 v1[2] + p11 w + p12 v2[2] is steered into each band at w = 1 through v2[2]
XI_TARGETS = [0.0, 3e-11, 1e-8, 9.9e-6, 1.01e-5, 1e-4, 9.9e-3, 1.01e-2]
XI_W = 1.0

DOF = 5
DT = 0.5
P1_XY = (0.5, -0.25)
Q1, Q2 = (0.3, -1.2), (0.35, -1.22)
VELOCITIES = [((0.8, -0.5, 0.3, 0.2, -0.4), (0.6, -0.7, -0.2, 0.25, -0.3))]
# states at rest as well, for these translations and first headings (the reference costs 10 ms a row)
ZERO_VELOCITY_AT = (TRANSLATIONS[:2], (HEADINGS[0], HEADINGS[2]))

# the obstacle factor's robot and fields: a Pose2 base with two spheres, one off the origin; the planar ramps d = x and
# d = y on a grid whose nodes are exact doubles; epsilon so large that the hinge is on everywhere on the grid
SPHERES = [(0.0, 0.0, 0.25), (0.375, -0.125, 0.125)]       # (ox, oy, radius)
GRID_ORIGIN, GRID_CELL, GRID_N = (-64.0, -64.0), 0.5, 257
EPSILON = 100.0

CAP = 1e-12
GROUPS = ("prior.err", "prior.H1", "prior.H2", "prior.H3", "prior.H4", "interp.conf", "interp.vel",
          "obs.H1", "obs.H2", "obs.H3", "obs.H4")


def _second_pose(th1, t, w):
    p1 = ref.M(P1_XY + (th1,))
    p2 = ref.compose(p1, ref.M(t + (w,)))
    return [float(p2[0]), float(p2[1]), float(ref.principal(p2[2]))]


@functools.lru_cache(maxsize=None)
def cases():
    """dict(prior=(c1, v1, c2, v2) [Mp][5], interp=(c1, v1, c2, v2, tau [Mi], label [Mi]) ...) as float64 arrays"""
    prior, interp = [], []
    for w in W_VALUES:
        for t in TRANSLATIONS:
            for th1 in HEADINGS:
                c1 = list(P1_XY) + [th1] + list(Q1)
                c2 = _second_pose(th1, t, w) + list(Q2)
                v1, v2 = VELOCITIES[0]
                prior.append((c1, list(v1), c2, list(v2), w))
                for f in TAU_FRACTIONS:
                    interp.append((c1, list(v1), c2, list(v2), DT * f, w))
                    if t in ZERO_VELOCITY_AT[0] and th1 in ZERO_VELOCITY_AT[1]:      # xi == 0 exactly at w == 0, t == 0
                        interp.append((c1, [0.0] * DOF, c2, [0.0] * DOF, DT * f, w))
    # xi[2] in each band although w is not
    for target in XI_TARGETS:
        for f in TAU_FRACTIONS:
            tau = DT * f
            c = ref.gp_coef(DT, tau)
            for t in TRANSLATIONS:
                for th1 in HEADINGS:
                    c1 = list(P1_XY) + [th1] + list(Q1)
                    c2 = _second_pose(th1, t, XI_W) + list(Q2)
                    va, vb = (list(v) for v in VELOCITIES[0])
                    wx = ref.Log(ref.between(ref.M(c1[:3]), ref.M(c2[:3])))[2]
                    vb[2] = float((mpf(target) - c["l12"] * mpf(va[2]) - c["p11"] * wx) / c["p12"])
                    interp.append((c1, va, c2, vb, tau, XI_W))
    f64 = lambda k, rows: np.ascontiguousarray([r[k] for r in rows], dtype=np.float64)
    out = dict(prior=tuple(f64(k, prior) for k in range(5)), interp=tuple(f64(k, interp) for k in range(6)))
    # no case sits on the cut: the exact heading difference is at least 1e-12 away from +-pi
    for name in ("prior", "interp"):
        c1, _, c2 = out[name][:3]
        for a, b in zip(c1[:, 2], c2[:, 2]):
            assert abs(abs(ref.circular(b, a)) - mp.pi) > 1e-12
    return out


def ramp_fields():
    """(origin, cell, data_x, data_y): d = x and d = y on the grid"""
    x = GRID_ORIGIN[0] + GRID_CELL * np.arange(GRID_N)
    y = GRID_ORIGIN[1] + GRID_CELL * np.arange(GRID_N)
    return list(GRID_ORIGIN), GRID_CELL, np.tile(x[None, :], (GRID_N, 1)), np.tile(y[:, None], (1, GRID_N))


def base_model():
    import gpmp2_amd as g
    return g.Pose2MobileBaseModel(g.Pose2MobileBase(), [g.BodySphere(0, r, (ox, oy, 0.0)) for ox, oy, r in SPHERES])


# ------------------------------------------------------------------------------------------------ the reference
def _err(got, want, circular_at=()):
    """max |got - want| of one output against its mpf reference, evaluated in mpf; heading entries on the circle"""
    got, flat = np.asarray(got, dtype=np.float64).reshape(-1), []
    for row in want:
        flat.extend(row) if isinstance(row, (list, tuple)) else flat.append(row)
    assert got.size == len(flat)
    worst = mpf(0)
    for k, (g_, w_) in enumerate(zip(got, flat)):
        d = ref.circular(g_, w_) if k in circular_at else mpf(float(g_)) - w_
        worst = max(worst, abs(d))
    return float(worst)


@functools.lru_cache(maxsize=None)
def reference():
    """The exact outputs of every case, computed once: dict(prior=[(err, [H1..H4], scale)], interp=[(conf, vel, scale)],
    obs=[([H1..H4], dist, scale)], xi=[xi[2] of every interp case])."""
    cs = cases()
    out = dict(prior=[], interp=[], obs=[], xi=[])
    for c1, v1, c2, v2, _ in zip(*cs["prior"]):
        a = tuple(ref.M(x) for x in (c1, v1, c2, v2))
        scale = max(1.0, float(np.abs(np.concatenate([c1, v1, c2, v2])).max()))
        out["prior"].append((ref.gp_prior_error(DT, *a), ref.gp_prior_jacobians(DT, *a), scale))
    for c1, v1, c2, v2, tau, _ in zip(*cs["interp"]):
        a = tuple(ref.M(x) for x in (c1, v1, c2, v2))
        co = ref.gp_coef(DT, tau)
        scale = max(1.0, float(np.abs(np.concatenate([c1, v1, c2, v2])).max()))
        conf, vel = ref.interpolate(co, *a)
        out["interp"].append((conf, vel, scale))
        out["xi"].append(float(ref.interpolate_tangent(co, *a)))
        a3 = tuple(x[:3] for x in a)
        errs, dist = ref.ramp_errors(co, SPHERES, mpf(EPSILON), *a3)
        assert min(errs) > 0, "the hinge must be on"
        lim = GRID_ORIGIN[0] + GRID_CELL * (GRID_N - 1)
        assert all(GRID_ORIGIN[0] < d < lim for d in dist), "a sphere left the grid"
        scale3 = max(1.0, float(np.abs(np.concatenate([c1[:3], v1[:3], c2[:3], v2[:3]])).max()),
                     max(float(abs(d)) for d in dist) + GRID_CELL)
        out["obs"].append((ref.ramp_jacobians(co, SPHERES, mpf(EPSILON), *a3), errs, scale3))
    return out


# ------------------------------------------------------------------------------------------------ one measurement
def measure(impl, robot, sdf_x, sdf_y):
    """impl: the engine or the oracle; robot, sdf_x, sdf_y: its handles of base_model() and ramp_fields().
    -> dict(group -> e [cases of that group]); asserts that the hinge was on in every obstacle case."""
    cs, rf = cases(), reference()
    e = {g_: [] for g_ in GROUPS}
    c1, v1, c2, v2, _ = cs["prior"]
    err, H = impl.gp_prior_factor(DOF, True, DT, c1, v1, c2, v2)
    for m, (r_err, r_H, scale) in enumerate(rf["prior"]):
        e["prior.err"].append(_err(err[m], r_err) / scale)
        for k in range(4):
            e[f"prior.H{k + 1}"].append(_err(H[k][m], r_H[k]) / scale)
    c1, v1, c2, v2, tau, _ = cs["interp"]
    S = len(SPHERES)
    for t in sorted(set(tau)):
        sel = np.flatnonzero(tau == t)
        a = tuple(np.ascontiguousarray(x[sel]) for x in (c1, v1, c2, v2))
        conf, vel = impl.gp_interpolate(DOF, True, np.eye(DOF), DT, float(t), *a)
        a3 = tuple(np.ascontiguousarray(x[:, :3]) for x in a)
        ex, Hx = impl.obstacle_gp_factor(robot, sdf_x, EPSILON, np.eye(3), DT, float(t), *a3)
        ey, Hy = impl.obstacle_gp_factor(robot, sdf_y, EPSILON, np.eye(3), DT, float(t), *a3)
        assert ex.min() > 0 and ey.min() > 0, "the hinge must be on in every case"
        for i, m in enumerate(sel):
            r_conf, r_vel, scale = rf["interp"][m]
            e["interp.conf"].append(_err(conf[i], r_conf, circular_at=(2,)) / scale)
            e["interp.vel"].append(_err(vel[i], r_vel) / scale)
            r_H, _, scale3 = rf["obs"][m]
            for k in range(4):
                got = np.concatenate([Hx[k][i], Hy[k][i]])       # [2 S][3]: x-field spheres, then y-field spheres
                assert got.shape == (2 * S, 3)
                e[f"obs.H{k + 1}"].append(_err(got, r_H[k]) / scale3)
    # the interp groups were filled tau by tau: put them back in case order
    order = np.concatenate([np.flatnonzero(tau == t) for t in sorted(set(tau))])
    inv = np.argsort(order)
    for g_ in GROUPS:
        v = np.array(e[g_])
        e[g_] = v[inv] if g_.startswith(("interp", "obs")) else v
    return e


def handles(impl):
    origin, cell, dx, dy = ramp_fields()
    return impl.robot(base_model()), impl.sdf(origin, cell, dx), impl.sdf(origin, cell, dy)


BANDS = [("w = 0", 0.0, 0.0), ("(0, 1e-10)", 0.0, 1e-10), ("[1e-10, 1e-5]", 1e-10, 1e-5), ("(1e-5, 1e-2)", 1e-5, 1e-2),
         ("[1e-2, 0.1]", 1e-2, 0.1), ("(0.1, pi)", 0.1, 4.0)]


def band_of(w):
    w = abs(float(w))
    if w == 0.0:
        return 0
    if w < 1e-10:
        return 1
    if w <= 1e-5:
        return 2
    if w < 1e-2:
        return 3
    return 4 if w <= 0.1 else 5


def case_bands(group):
    """the band index of every case of a group: by the exact heading difference for the prior and the velocity, by the
    smaller of |w| and |xi[2]| for what goes through Exp"""
    cs, rf = cases(), reference()
    exact = lambda c: [float(ref.circular(b, a)) for a, b in zip(c[0][:, 2], c[2][:, 2])]
    if group.startswith("prior"):
        return np.array([band_of(w) for w in exact(cs["prior"])])
    w = exact(cs["interp"])
    if group == "interp.vel":
        return np.array([band_of(x) for x in w])
    return np.array([min(band_of(a), band_of(b)) for a, b in zip(w, rf["xi"])])
