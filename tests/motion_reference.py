"""The motion limits of include/gpmp2mi.h ("motion limits") restated in numpy on the CPU oracle: interpolate_traj (both
halves) -> sphere_centers (Jacobians) -> J v, the two acceleration formulas, the extrema with their indices.  Nothing here
imports the product for its answers.  Shared by tests/test_motion_cpu.py (oracle only), tests/test_gpu_motion.py (the
expectation of the device's scores) and scripts/motion_error.py (which adds a truth in np.longdouble)."""
import numpy as np

from gpmp2_amd import robots

import score_reference as ref
import self_reference as sr

VALUES = ("pos_margin", "vel_ratio", "acc_ratio", "point_speed", "time_scale")
KINDS = ("pos_margin", "vel_ratio", "acc_ratio", "point_speed")      # the four extrema, in the order of worst [B][4][2]

# The tolerance of the device's values (DESIGN.md "motion limits", measured by scripts/motion_error.py):
#   err(x, truth) = |x - truth| / max(1, |truth|);  e_gpu <= K * max(e_cpu, FLOOR) and e_gpu <= CAP
K, FLOOR, CAP = 8.0, 2.0 ** -52, 1e-12


def err(x, truth):
    """the mixed error the tolerance is stated in; inf where one side is finite and the other is not"""
    x, truth = np.asarray(x, dtype=np.longdouble), np.asarray(truth, dtype=np.longdouble)
    same = (x == truth) | (np.isnan(x) & np.isnan(truth))
    with np.errstate(invalid="ignore"):
        e = np.abs(x - truth) / np.maximum(1.0, np.abs(truth))
    return np.where(same, 0.0, np.where(np.isfinite(e), e, np.inf)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# Limits.  The Barrett WAM's joint ranges and round rate limits, every entry shifted by a small offset without structure
# so that no two quantities of a trajectory tie through the table (round, symmetric limits gave a 2e-9 near-tie).
_OFF = np.array([0.00141421, 0.00173205, 0.00223607, 0.00264575, 0.00331662, 0.00360555, 0.00412311])
WAM_LIMITS = dict(
    pos_down=np.array([-2.6, -2.0, -2.8, -0.9, -4.76, -1.6, -3.0]) - _OFF,
    pos_up=np.array([2.6, 2.0, 2.8, 3.1, 1.24, 1.6, 3.0]) + _OFF[::-1],
    vel=2.0 + 0.1 * _OFF, acc=20.0 + _OFF, point_speed=1.5 + 0.000577216)
WAM_ROUND = dict(pos_down=[-2.6, -2.0, -2.8, -0.9, -4.76, -1.6, -3.0], pos_up=[2.6, 2.0, 2.8, 3.1, 1.24, 1.6, 3.0],
                 vel=2.0, acc=20.0, point_speed=1.5)
NO_LIMITS = dict(pos_down=None, pos_up=None, vel=None, acc=None, point_speed=np.inf)


def expand(lim, D):
    """(down, up, vel, acc, point_speed) as [D] arrays with +-inf where there is no limit"""
    def vec(x, fill):
        if x is None:
            return np.full(D, fill)
        a = np.asarray(x, dtype=np.float64)
        return np.full(D, float(a)) if a.ndim == 0 else a.copy()
    return (vec(lim.get("pos_down"), -np.inf), vec(lim.get("pos_up"), np.inf), vec(lim.get("vel"), np.inf),
            vec(lim.get("acc"), np.inf), float(lim.get("point_speed", np.inf)))


def _extremum(val, evaluated, smallest):
    """val [B][n1][n2], evaluated bool (broadcastable): the extremum over the finite evaluated entries with its
    (i, j) -- the first in (i, j) order among equals --, the number of evaluated entries that are not finite, and the
    gap to the runner-up (nan when there is none)."""
    B, n1, n2 = val.shape
    ev = np.broadcast_to(evaluated, val.shape)
    fin = ev & np.isfinite(val)
    key = np.where(fin, val if smallest else -val, np.inf).reshape(B, n1 * n2)
    none = ~fin.reshape(B, -1).any(axis=1)
    if n1 * n2 == 0:
        return (np.full(B, np.inf if smallest else 0.0), np.full((B, 2), -1, dtype=np.int32), np.zeros(B, dtype=np.int32),
                np.full(B, np.nan))
    arg = key.argmin(axis=1)
    best = key[np.arange(B), arg]
    worst = np.stack([arg // n2, arg % n2], axis=1).astype(np.int32)
    worst[none] = -1
    value = np.where(none, np.inf if smallest else 0.0, best if smallest else -best)
    if n1 * n2 > 1:
        part = np.partition(key, 1, axis=1)
        with np.errstate(invalid="ignore"):
            gap = np.where(np.isfinite(part[:, 1]), part[:, 1] - part[:, 0], np.nan)
    else:
        gap = np.full(B, np.nan)
    return value, worst, (ev & ~fin).reshape(B, -1).sum(axis=1).astype(np.int32), gap


def acceleration_ends(t, dt, D, c6=6.0):
    """t [B][N+1][2D] -> [B][2N][D]: the acceleration of the interpolated mean at the two ends of every interval, row
    2 i + e (c6: the coefficient 6 of the formulas, for the slip test)"""
    x0, v0, x1, v1 = t[:, :-1, :D], t[:, :-1, D:], t[:, 1:, :D], t[:, 1:, D:]
    w = c6 / (dt * dt)
    a0 = w * (x1 - x0) - (4.0 * v0 + 2.0 * v1) / dt
    a1 = -(w * (x1 - x0)) + (2.0 * v0 + 4.0 * v1) / dt
    return np.stack([a0, a1], axis=2).reshape(t.shape[0], -1, D)


def _pose2_interpolate(x0, v0, x1, v1, l12, p11, p12, l22, p21, p22):
    """The Pose2 part ([..., 3] arrays) of GaussianProcessInterpolatorPose2Vector with GTSAM's Pose2 between / Logmap /
    Expmap / compose, in the dtype of its inputs: (pose, velocity)."""
    c1, s1 = np.cos(x0[..., 2]), np.sin(x0[..., 2])
    dx, dy = x1[..., 0] - x0[..., 0], x1[..., 1] - x0[..., 1]
    bx, by = c1 * dx + s1 * dy, -s1 * dx + c1 * dy
    dth = x1[..., 2] - x0[..., 2]
    w = np.arctan2(np.sin(dth), np.cos(dth))
    one = np.ones_like(w)

    def half(w):        # a = w / 2, sin a, cos a, sin(a) / a: the cancellation-free forms of csrc/device_math.h
        a = w / 2
        z = a == 0
        return a, np.sin(a), np.cos(a), np.where(z, one, np.sin(a) / np.where(z, one, a))

    a, _, ca, q = half(w)
    h = ca / q
    lg = np.stack([h * bx + a * by, -a * bx + h * by, w], axis=-1)
    xi = l12 * v0 + p11 * lg + p12 * v1
    a, sa, ca, q = half(xi[..., 2])
    A, Bq = q * ca, q * sa
    ex, ey = A * xi[..., 0] - Bq * xi[..., 1], Bq * xi[..., 0] + A * xi[..., 1]
    eth = np.arctan2(2 * sa * ca, (ca - sa) * (ca + sa))
    ce, se = np.cos(eth), np.sin(eth)
    pose = np.stack([x0[..., 0] + c1 * ex - s1 * ey, x0[..., 1] + s1 * ex + c1 * ey,
                     np.arctan2(s1 * ce + c1 * se, c1 * ce - s1 * se)], axis=-1)
    return pose, l22 * v0 + p21 * lg + p22 * v1


def hermite_states(t, dt, J, D, dtype=np.float64, slip=0.0, lie=False):
    """The checked states from the cubic Hermite closed form of the GP mean, [B][Md][2D] in `dtype`; support states are
    copies.  lie: the first three coordinates are a Pose2 and go through the Pose2 interpolator with the same scalars.
    slip: the relative mistake in the interpolation time u = tau / dt (for the slip test)."""
    t = np.asarray(t, dtype=dtype)
    B, N = t.shape[0], t.shape[1] - 1
    one = dtype(1)
    out = np.zeros((B, N * (J + 1) + 1, 2 * D), dtype=dtype)
    x0, v0, x1, v1 = t[:, :-1, :D], t[:, :-1, D:], t[:, 1:, :D], t[:, 1:, D:]
    h = dtype(dt)
    for j in range(J + 1):
        if j == 0:
            out[:, 0:N * (J + 1):J + 1] = t[:, :-1]
            continue
        u = dtype(j) / dtype(J + 1) * (one + dtype(slip))
        h00, h10 = 2 * u ** 3 - 3 * u ** 2 + one, u ** 3 - 2 * u ** 2 + u
        h01, h11 = -2 * u ** 3 + 3 * u ** 2, u ** 3 - u ** 2
        d00, d10, d01, d11 = 6 * u ** 2 - 6 * u, 3 * u ** 2 - 4 * u + one, -6 * u ** 2 + 6 * u, 3 * u ** 2 - 2 * u
        out[:, j:N * (J + 1):J + 1, :D] = h00 * x0 + h10 * h * v0 + h01 * x1 + h11 * h * v1
        out[:, j:N * (J + 1):J + 1, D:] = (d00 * x0 + d01 * x1) / h + d10 * v0 + d11 * v1
        if lie:
            pose, vel = _pose2_interpolate(x0[..., :3], v0[..., :3], x1[..., :3], v1[..., :3], h * h10, h01, h * h11, d10,
                                           d01 / h, d11)
            out[:, j:N * (J + 1):J + 1, :3] = pose
            out[:, j:N * (J + 1):J + 1, D:D + 3] = vel
    out[:, -1] = t[:, -1]
    return out


def depends(model):
    """bool [S][D]: the Jacobian columns that enter a sphere's speed: those of the joints its link hangs from (a column
    that is left out is zero, so for finite input this changes nothing; a non-finite velocity of a joint further out
    leaves the speed finite).  Written down for fixed-base arms, the kind the non-finite tests use: joint d moves link l
    iff d <= l.  The other kinds take every column."""
    D, S = model.dof(), model.nr_body_spheres()
    if isinstance(model.fk_model(), robots.Arm):
        link = np.array([sph.link_id for sph in model.spheres])
        return np.arange(D)[None, :] <= link[:, None]
    return np.ones((S, D), dtype=bool)


def motion_from_states(orc, model, ro, lim, dt, J, t, U, dtype=np.float64, c6=6.0):
    """The definitions on given checked states U [B][Md][2D] (any float dtype; the Jacobians come from the oracle at
    float64) -> dict of the seven outputs plus gap [B][4]."""
    D, S = model.dof(), model.nr_body_spheres()
    B, Md = U.shape[0], U.shape[1]
    free = 3 if ref.is_lie(model) else 0
    down, up, vel, acc, ps = expand(lim, D)
    q, v = U[:, :, :D], U[:, :, D:]
    coord = np.arange(D) >= free
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        lo = np.where(np.isfinite(down), q - down.astype(dtype), np.inf)
        hi = np.where(np.isfinite(up), up.astype(dtype) - q, np.inf)
        margin = np.where(np.isfinite(q), np.minimum(lo, hi), np.nan)
        pos = _extremum(margin, (np.isfinite(down) | np.isfinite(up)) & coord, True)
        vr = _extremum(np.abs(v) / vel.astype(dtype), np.isfinite(vel), False)
        a = acceleration_ends(np.asarray(t, dtype=dtype), dtype(dt), D, dtype(c6))
        ar = _extremum(np.abs(a) / acc.astype(dtype), np.isfinite(acc) & coord, False)
        q64 = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, D)
        _, Jc = orc.sphere_centers(ro, q64)                                   # [M][S][3][D]
        dep = depends(model)
        u = np.where(dep[None, :, None, :], Jc.astype(dtype) * v.reshape(-1, 1, 1, D), 0).sum(axis=3)
        speed = np.sqrt((u * u).sum(axis=2)).reshape(B, Md, S)
        sp = _extremum(speed, np.ones(S, dtype=bool), False)
        scale = np.maximum(np.maximum(vr[0], np.sqrt(ar[0])), sp[0] / dtype(ps))
    four = (pos, vr, ar, sp)
    return dict(pos_margin=pos[0], vel_ratio=vr[0], acc_ratio=ar[0], point_speed=sp[0], time_scale=scale,
                worst=np.stack([x[1] for x in four], axis=1), invalid=sum(x[2] for x in four).astype(np.int32),
                gap=np.stack([x[3] for x in four], axis=1))


def oracle_motion_score(orc, model, ro, lim, dt, J, traj):
    """traj [B][N+1][2D] -> dict: the seven per-row outputs in float64 on the oracle's checked states, plus gap [B][4]:
    the distance between each extremum and its runner-up (0: an exact tie, nan: no runner-up)"""
    D = model.dof()
    t = np.ascontiguousarray(traj, dtype=np.float64).reshape(-1, np.shape(traj)[-2], 2 * D)
    lie = ref.is_lie(model)
    with np.errstate(invalid="ignore", over="ignore"):
        U = orc.interpolate_traj(D, lie, None, dt, J, t)
        if not np.isfinite(t).all():
            # The oracle interpolates with dense Lambda / Psi matrices, whose zeros turn one non-finite coordinate into a
            # NaN in every coordinate of the state.  The definition is per coordinate (as k_interpolate_traj computes
            # it): where only that artefact made an entry non-finite, the closed form of the same mean stands in.
            H = hermite_states(t, dt, J, D, lie=lie)
            U = np.where(~np.isfinite(U) & np.isfinite(H), H, U)
    return motion_from_states(orc, model, ro, lim, dt, J, t, U)


def truth_motion_score(orc, model, ro, lim, dt, J, traj):
    """the same in np.longdouble from the Hermite closed form (the Pose2 interpolator with its scalars for the mobile
    kinds)"""
    D = model.dof()
    t = np.ascontiguousarray(traj, dtype=np.float64).reshape(-1, np.shape(traj)[-2], 2 * D)
    U = hermite_states(t, dt, J, D, np.longdouble, lie=ref.is_lie(model))
    return motion_from_states(orc, model, ro, lim, dt, J, t, U, np.longdouble)


def decided(exp, c):
    """rows whose `worst` entry c is compared: an exact tie (the rule decides it) or a gap above the value tolerance"""
    gap = exp["gap"][:, c]
    scale = np.maximum(1.0, np.abs(exp[KINDS[c]]))
    with np.errstate(invalid="ignore"):
        return ~((gap > 0) & (gap <= 2 * CAP * scale))


# ---------------------------------------------------------------------------------------------------------------------
# The inputs of tests/test_gpu_motion.py, built without a GPU so that tests/test_motion_cpu.py can judge them on the oracle.
def models():
    import gpmp2_amd as g
    m = dict(sr.models())
    m["arm3"] = lambda: g.generateArm("SimpleThreeLinksArm")
    m["point1"] = lambda: robots.RobotModel(robots.PointRobot(2, 1), [robots.BodySphere(0, 0.5, (0.0, 0.0, 0.0))])
    return m


def case_limits(name):
    if name == "wam":
        return WAM_LIMITS
    if name == "arm3":
        return dict(pos_down=[-1.00141, -2.50173, -np.inf], pos_up=[1.50223, np.inf, 2.00264], vel=[1.00331, np.inf, 1.5036],
                    acc=[4.00412, 5.00141, np.inf], point_speed=1.00173)
    if name == "point1":
        return dict(pos_down=[-3.00141, -np.inf], pos_up=[5.00173, 4.00223], vel=1.50264, acc=3.00331, point_speed=2.0036)
    if name == "config5":   # coordinates 0..2: limits that would dominate everything if they were applied
        return dict(pos_down=[-1e-3, -1e-3, -1e-3, -0.50141, -3.00173], pos_up=[1e-3, 1e-3, 1e-3, 3.00223, 3.10264],
                    vel=[0.80331, 0.6036, 1.20412, 1.50141, 1.70173], acc=[1e-6, 1e-6, 1e-6, 6.00223, 7.00264],
                    point_speed=1.20331)
    if name == "pr2":
        off = 0.001 * np.sqrt(np.arange(2, 20))
        return dict(pos_down=-2.0 - off, pos_up=2.5 + off[::-1], vel=0.5 + 0.1 * off, acc=2.0 + off, point_speed=0.750577)
    raise KeyError(name)


def case_dt(name):
    return 10.0 / 50 if name == "pr2" else sr.DELTA_T


def warped_traj(rows, N, dt):
    """rows: list of (start, end, amp) -> [B][N+1][2D]: start -> end along s = (i/N)^1.37 with a bump amp sin(pi s), the
    velocities its time derivative.  Unlike a plain sine bump it has no mirror symmetry in time, so that two intervals do
    not share an acceleration or a speed."""
    out = []
    for start, end, amp in rows:
        start, end, amp = (np.asarray(x, dtype=np.float64) for x in (start, end, amp))
        i = np.arange(N + 1)[:, None] / N
        s = i ** 1.37
        ds = 1.37 * i ** 0.37 / (N * dt)
        conf = start + (end - start) * s + np.sin(np.pi * s) * amp
        vel = ds * ((end - start) + np.pi * np.cos(np.pi * s) * amp)
        out.append(np.concatenate([conf, vel], axis=1))
    return np.ascontiguousarray(out)


def case_traj(name, N, B=3):
    """B rows of a case's robot; the PR2 rows are the `init` of score_reference.pr2_problem (no solve)"""
    dt = case_dt(name)
    rng = np.random.default_rng(11 + N)
    if name == "pr2":
        return np.ascontiguousarray(ref.pr2_problem(B=4).init)
    if name == "point1":
        return warped_traj([([-2.0, 1.0], [2.0, 3.0], [0.3, -0.2]), ([0.5, 0.25], [4.5, -3.75], [0.0, 0.1]),
                            ([1.0, 1.0], [1.0, 5.0], [0.2, 0.0])][:B], N, dt)
    if name == "arm3":
        return warped_traj([sr.FOLDED, sr.STRETCHED, ([0.3, 1.2, 2.0], [-0.4, 2.2, 1.1], [0.2, -0.3, 0.1])][:B], N, dt)
    if name == "wam":
        return warped_traj([(rng.uniform(-1.5, 1.5, 7), rng.uniform(-1.5, 1.5, 7), rng.uniform(-0.5, 0.5, 7))
                            for _ in range(B)], N, dt)
    if name == "config5":
        return warped_traj([([-1.0, 0.0, 1.5, 0.2, 2.4], [1.0, 0.5, 0.9, 2.6, 2.9], [0.0, 0.3, 0.2, 0.3, -0.2]),
                            ([0.0, 0.0, 0.0, 3.0, 2.0], [0.5, -0.5, 1.0, 2.2, 3.0], [0.1, 0.0, 0.0, 0.0, 0.2]),
                            ([0.3, 0.2, -1.0, 0.1, 0.2], [-0.3, 0.6, 1.0, 0.9, -0.7], [0.0, 0.0, 0.5, 0.0, 0.0])][:B], N, dt)
    raise KeyError(name)


# (robot, (N, J), B)
GPU_CASES = [("arm3", (10, 0), 3), ("arm3", (10, 3), 3), ("point1", (1, 0), 3), ("wam", (8, 7), 3),
             ("wam", (12, 4), 1), ("wam", (12, 4), 3), ("wam", (12, 4), 16), ("wam", (20, 5), 1), ("wam", (20, 5), 3),
             ("wam", (20, 5), 16), ("config5", (16, 3), 3), ("pr2", (50, 2), 4)]


# `worst` of the PR2 case: its rows are the straight-line / sine-bump `init` of pr2_problem with constant velocities, its
# arms are mirror images and inter_step 2 puts two checked states symmetrically into every interval, so its velocity
# ratios (kind 1) and point speeds (kind 3) tie to rounding in the reference itself.  For these two kinds of this case
# the share of skipped rows is not asserted, and `worst` is compared only where the gap is above the tolerance (a tie
# that is exact in one arithmetic need not be in another).  The values are compared like everywhere else.
SHARE_EXEMPT = {"pr2": (1, 3)}


def case_id(c):
    return f"{c[0]}-N{c[1][0]}J{c[1][1]}-B{c[2]}"


def constructed_rows(N, dt=sr.DELTA_T):
    """WAM rows [4][N+1][14] with known answers: 0: at rest except for a velocity at the first support state (the
    acceleration maximum is at (i = 0, e = 0)); 1: the same at the last one ((N-1, 1)); 2: at rest except that the last
    state moves joint 0 only, in a configuration where the last sphere of the description is the fastest (the speed
    maximum is at the last checked state and the last sphere); 3: a constant-velocity straight line with the same speed
    in every joint (with inter_step 0 and uniform limits exact ties everywhere: the lowest indices)."""
    D = 7
    rows = np.zeros((4, N + 1, 2 * D))
    rows[:, :, :D] = np.array([0.33, -0.55, -1.1, -1.16, 0.75, 0.99, 0.26])
    rows[0, 0, D + 2] = 0.75
    rows[1, N, D + 4] = -0.625
    rows[2, N, D + 0] = 0.5
    step = 0.0625                                     # dyadic: conf and velocity are exact, and so is every state
    rows[3, :, :D] = -0.5 + step * np.arange(N + 1)[:, None]
    rows[3, :, D:] = step / dt
    return rows
