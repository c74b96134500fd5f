"""The torque limits of include/gpmp2mi.h ("torque limits") restated in numpy: inverse dynamics of a fixed-base DH arm by
the classical LINK-FRAME TWO-PASS recursion (velocities and accelerations outward in each link's own frame, forces and
moments inward), in float64 and in np.longdouble (the truth), and the score rule over the checked states.  The device
uses another formulation (one outward pass in the world frame, O(n^2), no backward pass: csrc/torque_kernels.hip), so
the two share no expression.  The interpolation comes from the oracle, the Hermite closed form and the acceleration
formulas from tests/motion_reference.py.  Nothing here imports the product for its answers.  Shared by
tests/test_torque_cpu.py (which pins this file with facts that do not depend on it), tests/test_gpu_torque.py and
scripts/torque_error.py."""
import numpy as np

from gpmp2_amd import dynamics as tables
from gpmp2_amd import robots

import motion_reference as mr

VALUES = ("torque_ratio", "static_ratio", "torque_time_scale")
KINDS = ("torque_ratio", "static_ratio", "c2")          # the three extrema, in the order of worst [B][3][2]

# The tolerance of the device's values (DESIGN.md "torque limits", measured by scripts/torque_error.py ->
# profiles/torque_error.txt): err(x, truth) = |x - truth| / max(1, |truth|); e_gpu <= K * max(e_cpu, FLOOR) and
# e_gpu <= CAP.  K is the next power of two above the largest measured e_gpu / max(e_cpu, FLOOR); CAP is a condition.
K, FLOOR, CAP = 32.0, 2.0 ** -52, 1e-11
err = mr.err
SLIPS = ("no_gyro", "no_wdot_product", "gravity_base", "com_frame")


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _mv(M, v):
    return np.einsum("...ij,...j->...i", M, v)


def _inertia_matrix(six, dtype):
    ixx, iyy, izz, ixy, ixz, iyz = (dtype(x) for x in six)
    return np.array([[ixx, ixy, ixz], [ixy, iyy, iyz], [ixz, iyz, izz]], dtype=dtype)


def _joint_rotation(theta, alpha, dtype):
    """Rz(theta) Rx(alpha): frame j expressed in frame j-1, [M][3][3]"""
    c, s = np.cos(theta), np.sin(theta)
    ca, sa = np.cos(dtype(alpha)), np.sin(dtype(alpha))
    zero = np.zeros_like(c)
    return np.stack([np.stack([c, -s * ca, s * sa], axis=-1), np.stack([s, c * ca, -c * sa], axis=-1),
                     np.stack([zero, zero + sa, zero + ca], axis=-1)], axis=-2)


def link_frames(arm, q, dtype=np.float64):
    """World rotation [M][L][3][3] and origin [M][L][3] of every link frame (the DH frame behind joint j's transform),
    and the same of the base frame in front of joint 0, by composing Rz(theta) Tz(d) Tx(a) Rx(alpha)"""
    q = np.asarray(q, dtype=dtype).reshape(-1, arm.dof())
    base = np.asarray(arm.base_pose, dtype=dtype)
    R = np.broadcast_to(base[:3, :3], (q.shape[0], 3, 3))
    t = np.broadcast_to(base[:3, 3], (q.shape[0], 3))
    Rs, ts = [R], [t]
    for j in range(arm.dof()):
        th = q[:, j] + dtype(arm.theta_bias[j])
        Rj = _joint_rotation(th, arm.alpha[j], dtype)
        step = np.stack([dtype(arm.a[j]) * np.cos(th), dtype(arm.a[j]) * np.sin(th), np.zeros_like(th) + dtype(arm.d[j])], axis=-1)
        t = t + _mv(R, step)
        R = R @ Rj
        Rs.append(R)
        ts.append(t)
    return np.stack(Rs[1:], axis=1), np.stack(ts[1:], axis=1), Rs[0], ts[0]


def inverse_dynamics(arm, table, q, qd, qdd, dtype=np.float64, slip=None):
    """tau [M][D] = ID(q, qd, qdd) of the arm with the inertial table (dict: mass [L], com [L][3], inertia [L][6],
    gravity [3]) by the link-frame two-pass recursion.  slip: one of SLIPS, a planted mistake (for the slip test)."""
    D = arm.dof()
    q, qd, qdd = (np.asarray(x, dtype=dtype).reshape(-1, D) for x in (q, qd, qdd))
    M = q.shape[0]
    base = np.asarray(arm.base_pose, dtype=dtype)
    g = np.asarray(table.get("gravity", (0.0, 0.0, -9.81)), dtype=dtype)
    z0 = np.array([0, 0, 1], dtype=dtype)
    w, wd = np.zeros((M, 3), dtype=dtype), np.zeros((M, 3), dtype=dtype)
    # a base that accelerates upward at |g| stands in for gravity; it is expressed in the base frame
    vd = np.broadcast_to(-g if slip == "gravity_base" else base[:3, :3].T @ (-g), (M, 3))
    Rs, ps, rs, Fs, Ns = [], [], [], [], []
    for j in range(D):
        R = _joint_rotation(q[:, j] + dtype(arm.theta_bias[j]), arm.alpha[j], dtype)
        RT = np.swapaxes(R, -1, -2)
        ca, sa = np.cos(dtype(arm.alpha[j])), np.sin(dtype(arm.alpha[j]))
        p = np.array([dtype(arm.a[j]), dtype(arm.d[j]) * sa, dtype(arm.d[j]) * ca], dtype=dtype)   # o_{j-1} -> o_j in frame j
        zq, zqq = z0 * qd[:, j:j + 1], z0 * qdd[:, j:j + 1]
        product = 0 if slip == "no_wdot_product" else _cross(w, zq)
        w_new = _mv(RT, w + zq)
        wd = _mv(RT, wd + zqq + product)
        w = w_new
        vd = _cross(wd, p) + _cross(w, _cross(w, p)) + _mv(RT, vd)
        r = np.asarray(table["com"][j], dtype=dtype)
        if slip == "com_frame":
            r = _mv(RT, np.broadcast_to(r, (M, 3)))
        vc = _cross(wd, r) + _cross(w, _cross(w, r)) + vd
        I = _inertia_matrix(table["inertia"][j], dtype)
        gyro = 0 if slip == "no_gyro" else _cross(w, _mv(I, w))
        Rs.append(R)
        ps.append(p)
        rs.append(r)
        Fs.append(dtype(table["mass"][j]) * vc)
        Ns.append(_mv(I, wd) + gyro)
    tau = np.zeros((M, D), dtype=dtype)
    f, n = np.zeros((M, 3), dtype=dtype), np.zeros((M, 3), dtype=dtype)
    for j in reversed(range(D)):
        if j < D - 1:
            f, n = _mv(Rs[j + 1], f), _mv(Rs[j + 1], n)
        n = Ns[j] + n + _cross(ps[j] + rs[j], Fs[j]) + _cross(ps[j], f)      # the moment about o_{j-1}, frame j
        f = Fs[j] + f
        tau[:, j] = (n * Rs[j][:, 2, :]).sum(axis=-1)                       # z_{j-1} in frame j is the third row of R_j
    return tau


def checked_inputs(orc, D, dt, J, traj, dtype=np.float64):
    """traj [B][N+1][2D] -> the checked states U [B][Md][2D], the acceleration of side 0 at every state [B][Md][D] (the
    right-sided value at a support state, the left-sided one at the last state), that of side 1 [B][Md][D] (NaN where
    there is none) and the mask [Md] of the states with a side 1.  float64: the oracle's interpolation; else the
    Hermite closed form in `dtype`."""
    t = np.ascontiguousarray(traj, dtype=np.float64).reshape(-1, np.shape(traj)[-2], 2 * D)
    B, N = t.shape[0], t.shape[1] - 1
    if dtype is np.float64:
        with np.errstate(invalid="ignore", over="ignore"):
            U = orc.interpolate_traj(D, False, None, dt, J, t)
            if not np.isfinite(t).all():     # per coordinate, as the device interpolates (motion_reference says why)
                H = mr.hermite_states(t, dt, J, D)
                U = np.where(~np.isfinite(U) & np.isfinite(H), H, U)
    else:
        U = mr.hermite_states(t, dt, J, D, dtype)
    A = mr.acceleration_ends(np.asarray(t, dtype=dtype), dtype(dt), D, dtype(6.0))
    a0, a1 = A[:, 0::2], A[:, 1::2]
    Md = N * (J + 1) + 1
    first = np.zeros((B, Md, D), dtype=dtype)
    second = np.full((B, Md, D), np.nan, dtype=dtype)
    has2 = np.zeros(Md, dtype=bool)
    for j in range(J + 1):
        idx = np.arange(N) * (J + 1) + j
        first[:, idx] = a0 if j == 0 else a0 + (a1 - a0) * (dtype(j) / dtype(J + 1))
    first[:, -1] = a1[:, -1]
    sup = np.arange(1, N) * (J + 1)
    second[:, sup] = a1[:, :-1]
    has2[sup] = True
    return U, first, second, has2


def torque_from_inputs(arm, table, U, first, second, has2, dtype=np.float64, slip=None):
    """The definitions on given checked states and accelerations -> dict of the six outputs, c2 [B] (the square of
    torque_time_scale before the static test) and gap [B][3] (the distance of each extremum to its runner-up)."""
    D = arm.dof()
    B, Md = U.shape[0], U.shape[1]
    q, v = U[:, :, :D].reshape(-1, D), U[:, :, D:].reshape(-1, D)
    zero = np.zeros_like(q)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        tg = inverse_dynamics(arm, table, q, zero, zero, dtype, slip).reshape(B, Md, D)
        t1 = inverse_dynamics(arm, table, q, v, first.reshape(-1, D), dtype, slip).reshape(B, Md, D)
        t2 = np.full((B, Md, D), np.nan, dtype=dtype)
        if has2.any():
            sel = np.broadcast_to(has2[None, :], (B, Md)).reshape(-1)
            t2[:, has2] = inverse_dynamics(arm, table, q[sel], v[sel], second[:, has2].reshape(-1, D), dtype,
                                           slip).reshape(B, -1, D)
        lim = table.get("torque")
        L = np.full(D, np.inf, dtype=dtype) if lim is None else np.asarray(lim, dtype=dtype)
        limited = np.isfinite(L)

        def r_of(t):
            m = t - tg
            den = np.where(m > 0, L - tg, L + tg)
            r = np.where(m == 0, 0, np.where(den > 0, np.abs(m) / den, np.nan))
            return np.where(np.isfinite(t) & np.isfinite(tg), r, np.nan)

        def ratio(t):
            return np.where(np.isfinite(t), np.abs(t) / L, np.nan)

        both = lambda f: np.fmax(f(t1), f(t2))          # a NaN side (none, or not finite) leaves the other
        tr = mr._extremum(both(ratio), limited, False)
        sr = mr._extremum(ratio(tg), limited, False)
        cr = mr._extremum(both(r_of), limited, False)
        scale = np.where(sr[0] >= 1, np.inf, np.sqrt(cr[0]))
    invalid = (~np.isfinite(t1)).reshape(B, -1).sum(axis=1) + (~np.isfinite(t2[:, has2])).reshape(B, -1).sum(axis=1)
    three = (tr, sr, cr)
    return dict(torque_ratio=tr[0], static_ratio=sr[0], torque_time_scale=scale, c2=cr[0],
                worst=np.stack([x[1] for x in three], axis=1), invalid=invalid.astype(np.int32), tau=t1, tau_g=tg,
                tau_left=t2, gap=np.stack([x[3] for x in three], axis=1))


def reference_torque_score(orc, model, table, dt, J, traj, slip=None):
    """the float64 reference on the oracle's checked states"""
    D = model.dof()
    return torque_from_inputs(model.fk_model(), table, *checked_inputs(orc, D, dt, J, traj), slip=slip)


def truth_torque_score(orc, model, table, dt, J, traj):
    """the same in np.longdouble from the Hermite closed form"""
    D = model.dof()
    return torque_from_inputs(model.fk_model(), table, *checked_inputs(orc, D, dt, J, traj, np.longdouble), np.longdouble)


def decided(exp, c):
    """rows whose `worst` entry c is compared: an exact tie (the rule decides it) or a gap above the value tolerance"""
    gap = exp["gap"][:, c]
    scale = np.maximum(1.0, np.abs(exp[KINDS[c]]))
    with np.errstate(invalid="ignore"):
        return ~((gap > 0) & (gap <= 2 * CAP * scale))


# ---------------------------------------------------------------------------------------------------------------------
# The inputs of tests/test_gpu_torque.py, built without a GPU so that tests/test_torque_cpu.py can judge them.
def _tilt(rx, ry, t):
    cx, sx, cy, sy = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Ry @ Rx, t
    return T


WAM_BIAS = np.array([0.11, -0.23, 0.05, 0.31, -0.17, 0.07, 0.29])


def models():
    import gpmp2_amd as g
    wam = g.generateArm("WAMArm")
    w = wam.fk_model()
    pi = np.pi
    return dict(
        one=lambda: robots.RobotModel(robots.Arm(1, [0.4], [0.0], [0.05], _tilt(0.3, -0.2, [0.1, 0.0, 0.2])),
                                      [robots.BodySphere(0, 0.05, (-0.2, 0.0, 0.0))]),
        two=lambda: g.generateArm("SimpleTwoLinksArm"),
        wam=lambda: robots.RobotModel(robots.Arm(7, w.a, w.alpha, w.d, _tilt(0.35, -0.5, [0.2, -0.1, 0.4]), WAM_BIAS),
                                      wam.spheres),
        arm8=lambda: robots.RobotModel(
            robots.Arm(8, [0.0, 0.3, 0.05, 0.0, 0.25, 0.0, 0.04, 0.1], [-pi / 2, 0.0, pi / 2, -pi / 2, 0.3, pi / 2, -pi / 2, 0.0],
                       [0.2, 0.0, 0.1, 0.3, 0.0, 0.15, 0.0, 0.05], _tilt(-0.4, 0.25, [0.0, 0.3, 0.1]),
                       [0.2, -0.1, 0.0, 0.3, 0.15, -0.25, 0.1, 0.05]),
            [robots.BodySphere(j, 0.04, (0.0, 0.0, 0.0)) for j in range(8)]))


def case_table(name):
    """the inertial table of a case: dict(mass, com, inertia, gravity, torque)"""
    if name == "one":
        return dict(mass=np.array([1.7]), com=np.array([[-0.18, 0.01, 0.02]]),
                    inertia=np.array([tables.box_inertia(1.7, 0.4, 0.06, 0.05, 2e-4, -1e-4, 5e-5)]),
                    gravity=np.array([0.0, 0.0, -9.81]), torque=np.array([9.00141]))
    if name == "two":     # planar in the world's x-y plane: gravity along -y, the centres of mass on the links' x axes
        return dict(mass=np.array([1.3, 0.9]), com=np.array([[-0.22, 0.0, 0.0], [-0.27, 0.0, 0.0]]),
                    inertia=np.array([[0.002, 0.03, 0.031, 0.0, 0.0, 0.0], [0.001, 0.02, 0.0205, 0.0, 0.0, 0.0]]),
                    gravity=np.array([0.0, -9.81, 0.0]), torque=np.array([14.00173, 4.00223]))
    if name == "wam":
        t = tables.illustrative_wam()
        return dict(t, gravity=np.array([0.0, 0.0, -9.81]), torque=t["torque"] + mr._OFF)
    if name == "arm8":
        rng = np.random.default_rng(8)
        mass = np.array([4.1, 3.2, 2.6, 1.9, 1.2, 0.8, 0.5, 0.3])
        edges = rng.uniform(0.05, 0.3, (8, 3))
        prod = rng.uniform(-1.0, 1.0, (8, 3)) * 0.02 * mass[:, None] * 0.01
        return dict(mass=mass, com=rng.uniform(-0.08, 0.08, (8, 3)),
                    inertia=np.array([tables.box_inertia(m, *e, *p) for m, e, p in zip(mass, edges, prod)]),
                    gravity=np.array([0.3, -0.2, -9.7]),
                    torque=np.array([60.0, 55.0, 40.0, 30.0, 18.0, 9.0, 5.0, 2.0]) + 0.001 * np.sqrt(np.arange(2, 10)))
    raise KeyError(name)


DURATION = 2.5      # seconds, every case: |q'| stays below about 2, |q''| below about 20


def case_dt(N):
    return DURATION / N


def case_traj(name, N, B=3):
    """B rows of a case's robot: mr.warped_traj between random configurations"""
    D = dict(one=1, two=2, wam=7, arm8=8)[name]
    rng = np.random.default_rng(100 * D + N)
    return mr.warped_traj([(rng.uniform(-1.2, 1.2, D), rng.uniform(-1.2, 1.2, D), rng.uniform(-0.4, 0.4, D))
                           for _ in range(B)], N, case_dt(N))


# (N, J): Md = 13, 63, 64 and 65, the tile edge of SCORE_TILE = 64 on both sides
SHAPES = ((12, 0), (31, 1), (9, 6), (8, 7))
GPU_CASES = [(name, NJ, 3) for name in ("one", "two", "wam", "arm8") for NJ in SHAPES]


def case_id(c):
    return f"{c[0]}-N{c[1][0]}J{c[1][1]}-B{c[2]}"


REST = np.array([0.33, -0.55, -1.1, -1.16, 0.75, 0.99, 0.26])
PEAK_STATE, PEAK_JOINT = 5, 1


def constructed_rows(N, dt, tau_g_sign):
    """WAM rows [4][N+1][14] with known answers: 0: at rest; 1 and 2: at rest except for a velocity of joint PEAK_JOINT
    at support state PEAK_STATE, whose Hermite acceleration is +-4 v / dt on the two sides of that state and smaller
    everywhere else; in row 1 the right-sided value has the sign of the gravity torque (tau_g_sign) and is the peak, in
    row 2 the left-sided one; 3: at rest, with a NaN in one coordinate of one support state."""
    rows = np.zeros((4, N + 1, 14))
    rows[:, :, :7] = REST
    v = 0.125 * tau_g_sign
    rows[1, PEAK_STATE, 7 + PEAK_JOINT] = -v      # right side: -4 (-v) / dt
    rows[2, PEAK_STATE, 7 + PEAK_JOINT] = v       # left side:  +4 v / dt
    rows[3, 3, 4] = np.nan
    return rows


def planar_two_link(table, q, qd, qdd):
    """The textbook closed form of the planar two-link arm (link lengths 0.5, gravity along -y, joint angles from the
    x axis): tau [M][2]"""
    q, qd, qdd = (np.asarray(x, dtype=np.longdouble).reshape(-1, 2) for x in (q, qd, qdd))
    m1, m2 = (np.longdouble(x) for x in table["mass"])
    l1 = np.longdouble(0.5)
    lc1, lc2 = l1 + np.longdouble(table["com"][0][0]), l1 + np.longdouble(table["com"][1][0])
    I1, I2 = np.longdouble(table["inertia"][0][2]), np.longdouble(table["inertia"][1][2])
    g = -np.longdouble(table["gravity"][1])
    c2, s2 = np.cos(q[:, 1]), np.sin(q[:, 1])
    M11 = m1 * lc1 ** 2 + m2 * (l1 ** 2 + lc2 ** 2 + 2 * l1 * lc2 * c2) + I1 + I2
    M12 = m2 * (lc2 ** 2 + l1 * lc2 * c2) + I2
    M22 = m2 * lc2 ** 2 + I2
    h = -m2 * l1 * lc2 * s2
    g1 = (m1 * lc1 + m2 * l1) * g * np.cos(q[:, 0]) + m2 * lc2 * g * np.cos(q[:, 0] + q[:, 1])
    g2 = m2 * lc2 * g * np.cos(q[:, 0] + q[:, 1])
    t1 = M11 * qdd[:, 0] + M12 * qdd[:, 1] + h * (2 * qd[:, 0] * qd[:, 1] + qd[:, 1] ** 2) + g1
    t2 = M12 * qdd[:, 0] + M22 * qdd[:, 1] - h * qd[:, 0] ** 2 + g2
    return np.stack([t1, t2], axis=1)


def energy(arm, table, q, qd, dtype=np.longdouble):
    """kinetic + potential energy [M] from forward kinematics alone: the link frames give the centres of mass, the joint
    axes and origins, hence the velocity of every centre of mass and the angular velocity of every link"""
    D = arm.dof()
    q, qd = (np.asarray(x, dtype=dtype).reshape(-1, D) for x in (q, qd))
    R, t, Rb, tb = link_frames(arm, q, dtype)
    g = np.asarray(table.get("gravity", (0.0, 0.0, -9.81)), dtype=dtype)
    z = [Rb[:, :, 2]] + [R[:, j, :, 2] for j in range(D - 1)]
    o = [tb] + [t[:, j] for j in range(D - 1)]
    E = np.zeros(q.shape[0], dtype=dtype)
    for j in range(D):
        c = t[:, j] + _mv(R[:, j], np.asarray(table["com"][j], dtype=dtype))
        vc = sum(_cross(z[k], c - o[k]) * qd[:, k:k + 1] for k in range(j + 1))
        w = sum(z[k] * qd[:, k:k + 1] for k in range(j + 1))
        wl = _mv(np.swapaxes(R[:, j], -1, -2), w)
        I = _inertia_matrix(table["inertia"][j], dtype)
        m = dtype(table["mass"][j])
        E = E + m * (vc * vc).sum(axis=-1) / 2 + (wl * _mv(I, wl)).sum(axis=-1) / 2 - m * (c * g).sum(axis=-1)
    return E
