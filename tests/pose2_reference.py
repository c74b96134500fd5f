"""The exact Pose2 maps and what the planner builds on them, in mpmath at 60 digits.  TEST INFRASTRUCTURE ONLY.

Nothing here has a small-angle branch: Exp and Log are the closed forms (1 - cos w taken as 2 sin^2(w / 2), which does
not cancel), evaluated with far more digits than a double holds, and the w == 0 limit is taken exactly.  No derivative
formula is restated: every Jacobian is a central difference with step 1e-25 taken through the state's chart --
pose coordinates compose (dx, dy, dtheta) on the right, velocities and arm joints add -- so its truncation error is
O(1e-50) and its rounding error O(1e-33).  (tests/test_pose2_reference_cpu.py pins this against the closed-form inverse
right Jacobian at O(1) angles.)

All inputs are taken as the exact doubles the kernels receive: mpf(float) is exact.

States are tuples (x, y, theta, q...) of mpf; a pose is the first three.  Headings are kept unwrapped inside and brought
to the principal value (-pi, pi] by Log and by `principal`.
"""
from __future__ import annotations

import functools

from mpmath import mp, mpf

mp.dps = 60
STEP = mpf(10) ** -25
PI, TWO_PI = +mp.pi, 2 * mp.pi


def M(x):
    """a tuple of exact mpf from doubles"""
    return tuple(mpf(float(v)) for v in x)


def principal(th):
    """the heading in (-pi, pi]"""
    if -PI < th <= PI:
        return th
    r = th - TWO_PI * mp.floor(th / TWO_PI)       # [0, 2 pi)
    return r - TWO_PI if r > PI else r


def circular(a, b):
    """a - b on the circle, in (-pi, pi]"""
    return principal(mpf(a) - mpf(b))


# ------------------------------------------------------------------------------------------------ the group
def compose(a, b):
    c, s = mp.cos_sin(a[2])
    return (a[0] + c * b[0] - s * b[1], a[1] + s * b[0] + c * b[1], a[2] + b[2])


def inverse(a):
    c, s = mp.cos_sin(a[2])
    return (-(c * a[0] + s * a[1]), -(-s * a[0] + c * a[1]), -a[2])


def between(a, b):
    return compose(inverse(a), b)


def _V(w):
    """t = V(w) v of Exp:  V = [A -B; B A],  A = sin w / w,  B = (1 - cos w) / w = sin^2(w / 2) / (w / 2): the differences
    below take B at w = 1e-25, where 1 - cos w itself would keep 10 of 60 digits.  The limit at 0 is exact."""
    if w == 0:
        return mpf(1), mpf(0)
    s = mp.sin(w / 2)
    return mp.sin(w) / w, 2 * s * s / w


def Exp(v):
    A, B = _V(v[2])
    return (A * v[0] - B * v[1], B * v[0] + A * v[1], v[2])


def Log(p):
    w = principal(p[2])
    A, B = _V(w)
    det = A * A + B * B
    return ((A * p[0] + B * p[1]) / det, (-B * p[0] + A * p[1]) / det, w)


# ------------------------------------------------------------------------------------------------ charts
def retract(x, d):
    """state (pose, q...) (+) d: the pose composes (dx, dy, dtheta) on the right, the rest adds"""
    p = compose(x[:3], d[:3])
    return p + tuple(a + b for a, b in zip(x[3:], d[3:]))


def local(x, y):
    """the coordinates of y in the chart at x: retract(x, local(x, y)) == y"""
    b = between(x[:3], y[:3])
    return (b[0], b[1], principal(b[2])) + tuple(q - p for p, q in zip(x[3:], y[3:]))


def add(x, d):
    return tuple(a + b for a, b in zip(x, d))


def difference(f, args, kinds, out_chart=None):
    """Central differences of f(*args) -> tuple, one Jacobian [rows][cols] per argument.  kinds[i] is 'state' (through
    retract) or 'vector' (additive).  out_chart: None for an additive output, or a function (y0, y) -> coordinates."""
    jacs = []
    y0 = f(*args)
    for i, (a, kind) in enumerate(zip(args, kinds)):
        n = len(a)
        cols = []
        for j in range(n):
            out = []
            for sgn in (1, -1):
                d = tuple(sgn * STEP if k == j else mpf(0) for k in range(n))
                moved = retract(a, d) if kind == "state" else add(a, d)
                y = f(*(args[:i] + (moved,) + args[i + 1:]))
                out.append(y if out_chart is None else out_chart(y0, y))
            cols.append([(p - m) / (2 * STEP) for p, m in zip(*out)])
        jacs.append([[cols[j][r] for j in range(n)] for r in range(len(cols[0]))])
    return jacs


# ------------------------------------------------------------------------------------------------ the GP
def gp_coef(dt, tau):
    """Lambda / Psi scalars of one sub-step with Qc factored out, from the doubles dt and tau (as gp_coef_dev does, in
    exact arithmetic): dict l11 l12 l21 l22 p11 p12 p21 p22"""
    dt, tau = mpf(float(dt)), mpf(float(tau))
    a0, a1, r = tau ** 3 / 3, tau ** 2 / 2, dt - tau
    w0, w1, w3 = 12 / dt ** 3, -6 / dt ** 2, 4 / dt
    t0, t1, t2, t3 = a0 + a1 * r, a1, a1 + tau * r, tau
    c = dict(p11=t0 * w0 + t1 * w1, p12=t0 * w1 + t1 * w3, p21=t2 * w0 + t3 * w1, p22=t2 * w1 + t3 * w3)
    c.update(l11=1 - c["p11"], l12=tau - (c["p11"] * dt + c["p12"]), l21=-c["p21"],
             l22=1 - (c["p21"] * dt + c["p22"]))
    return c


@functools.lru_cache(maxsize=4)
def _between_log(x1, x2):
    return Log(between(x1[:3], x2[:3])) + tuple(b - a for a, b in zip(x1[3:], x2[3:]))


def gp_prior_error(dt, x1, v1, x2, v2):
    """GaussianProcessPriorPose2Vector::evaluateError: [Log(x1^-1 x2) - v1 dt ; v2 - v1]"""
    dt = mpf(float(dt))
    r = _between_log(x1, x2)
    return tuple(a - b * dt for a, b in zip(r, v1)) + tuple(b - a for a, b in zip(v1, v2))


def gp_prior_jacobians(dt, x1, v1, x2, v2):
    """H1..H4 [2D][D] of the prior error, differenced"""
    return difference(lambda a, b, c, d: gp_prior_error(dt, a, b, c, d), (x1, v1, x2, v2),
                      ("state", "vector", "state", "vector"))


def interpolate(c, x1, v1, x2, v2):
    """GaussianProcessInterpolatorPose2Vector: (pose x1 (+) Exp(xi), velocity), c = gp_coef(dt, tau)"""
    r = _between_log(x1, x2)
    xi = tuple(c["l12"] * a + c["p11"] * b + c["p12"] * d for a, b, d in zip(v1, r, v2))
    conf = compose(x1[:3], Exp(xi[:3])) + tuple(a + b for a, b in zip(x1[3:], xi[3:]))
    vel = tuple(c["l22"] * a + c["p21"] * b + c["p22"] * d for a, b, d in zip(v1, r, v2))
    return conf, vel


def interpolate_tangent(c, x1, v1, x2, v2):
    """xi[2], the heading part of the interpolated tangent (which band Exp and its derivative work in)"""
    r = _between_log(x1, x2)
    return c["l12"] * v1[2] + c["p11"] * r[2] + c["p12"] * v2[2]


def interpolate_jacobians(c, x1, v1, x2, v2):
    """M1..M4 [D][D] of the interpolated state in its own chart, differenced"""
    return difference(lambda a, b, cc, d: interpolate(c, a, b, cc, d)[0], (x1, v1, x2, v2),
                      ("state", "vector", "state", "vector"), out_chart=local)


# ------------------------------------------------------------------------------------------------ the ramp obstacle
def ramp_errors(c, spheres, eps, x1, v1, x2, v2):
    """The hinge errors of a Pose2 base with `spheres` [(ox, oy, radius)] against the two planar ramp fields d = x and
    d = y, at the interpolated pose, hinge taken as ON: (eps + r - x_s ..., eps + r - y_s ...), and the distances."""
    p = interpolate(c, x1, v1, x2, v2)[0]
    cs, sn = mp.cos_sin(p[2])
    xs = [p[0] + cs * ox - sn * oy for ox, oy, _ in spheres]
    ys = [p[1] + sn * ox + cs * oy for ox, oy, _ in spheres]
    ex = tuple(eps + r - x for x, (_, _, r) in zip(xs, spheres))
    ey = tuple(eps + r - y for y, (_, _, r) in zip(ys, spheres))
    return ex + ey, tuple(xs) + tuple(ys)


def ramp_jacobians(c, spheres, eps, x1, v1, x2, v2):
    """H1..H4 [2 S][3] of ramp_errors (rows: x-field spheres, then y-field spheres), differenced"""
    return difference(lambda a, b, cc, d: ramp_errors(c, spheres, eps, a, b, cc, d)[0], (x1, v1, x2, v2),
                      ("state", "vector", "state", "vector"))
