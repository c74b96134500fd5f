"""The exact SO(3) / SE(3) maps and what the workspace factors build on them, in mpmath at 60 digits.  TEST
INFRASTRUCTURE ONLY.

Nothing here has a small-angle or a near-pi branch of the kind a double needs: Exp is Rodrigues' formula with
1 - cos t taken as 2 sin^2(t / 2) and t - sin t by its series below 1/2, Log is atan2 of the skew part's norm and the
trace (60 digits keep the axis to 1e-45 even at pi - 1e-9), and only the exact limits t == 0 and t == pi are taken
apart.  Log is the principal value, |omega| <= pi, the sign at exactly pi being the one with the largest axis component
positive.  No derivative formula is restated: every Jacobian is a central difference with step 1e-25 through the
chart T * Exp(delta), delta = [omega; u] in GTSAM's order.  (tests/test_lie3_reference_cpu.py pins this against the
closed-form inverse right Jacobian at O(1) angles.)

All inputs are the exact doubles the kernels receive: mpf(float) is exact.  The rotation blocks of such inputs are
therefore not exactly orthonormal: `rel` forms Rd^T Rm exactly and Log is taken of ITS NEAREST ROTATION, the
orthogonal polar factor (Newton's iteration X <- (X + X^-T) / 2, which converges quadratically from 1e-16, or from the
1e-8 of a float32 rounding).  Any other sensible definition -- the polar factors of Rd and Rm first, say -- differs by
O(1e-16), which is inside the FLOOR of the GPU test.

A rotation is an mp.matrix 3x3, a pose the pair (R, t) with t an mp.matrix 3x1.
"""
from __future__ import annotations

import functools

from mpmath import mp, mpf

mp.dps = 60
STEP = mpf(10) ** -25
PI = +mp.pi
EYE = mp.eye(3)


def M(x):
    """a tuple of exact mpf from doubles"""
    return tuple(mpf(float(v)) for v in x)


def mat(a):
    """an exact mp.matrix from a double array [r][c] (or [r])"""
    rows = [list(r) if hasattr(r, "__len__") else [r] for r in a]
    return mp.matrix([[mpf(float(v)) for v in r] for r in rows])


def vec(x):
    return mp.matrix([[mpf(v)] for v in x])


def skew(w):
    return mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def norm(w):
    return mp.sqrt(sum(x * x for x in w))


def pose_of(T):
    """(R, t) from a double 4x4"""
    return mat([list(T[i][:3]) for i in range(3)]), vec([mpf(float(T[i][3])) for i in range(3)])


# ------------------------------------------------------------------------------------------------ SO(3)
def _series(t2, first):
    """sum_k (-1)^k t^2k / (2k + first)!, to the last digit"""
    s, term, k = mpf(0), mpf(1) / mp.factorial(first), 0
    while abs(term) > mpf(10) ** -75:
        s += term
        k += 1
        term = -term * t2 / ((2 * k + first - 1) * (2 * k + first))
    return s


def abc(t):
    """A = sin t / t, B = (1 - cos t) / t^2, C = (t - sin t) / t^3"""
    if t == 0:
        return mpf(1), mpf(1) / 2, mpf(1) / 6
    h = mp.sin(t / 2)
    C = _series(t * t, 3) if t < 0.5 else (t - mp.sin(t)) / t ** 3
    return mp.sin(t) / t, 2 * h * h / (t * t), C


def Exp(w):
    w = list(w)
    t = norm(w)
    A, B, _ = abc(t)
    W = skew(w)
    return EYE + A * W + B * (W * W)


def polar(X):
    """the nearest rotation of a matrix that is one to 1e-7 or better"""
    for _ in range(12):
        Y = (X + (X ** -1).T) / 2
        moved = max(abs(x) for x in Y - X)
        X = Y
        if moved < mpf(10) ** -35:        # quadratic: the next step would move by 1e-70
            return X
    raise ArithmeticError("polar: not a near-rotation")


def Log(R):
    """omega of an exact rotation"""
    v = [(R[2, 1] - R[1, 2]) / 2, (R[0, 2] - R[2, 0]) / 2, (R[1, 0] - R[0, 1]) / 2]
    s, c = norm(v), (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2
    t = mp.atan2(s, c)
    if s > mpf(10) ** -30:
        return tuple(x * t / s for x in v)
    if c > 0:
        return tuple(v)               # t / sin t = 1 + O(1e-60)
    # pi to 1e-30: the axis from the symmetric part (R + R^T) / 2 = c I + (1 - c) a a^T, largest component positive
    i = max(range(3), key=lambda k: R[k, k])
    ai = mp.sqrt((R[i, i] - c) / (1 - c))
    a = [(R[i, j] + R[j, i]) / (2 * (1 - c) * ai) for j in range(3)]
    a[i] = ai
    return tuple(t * x for x in a)


def rel(Rd, Rm):
    """the nearest rotation of Rd^T Rm, formed exactly from the doubles"""
    return polar(Rd.T * Rm)


# ------------------------------------------------------------------------------------------------ SE(3)
def V(w):
    t = norm(w)
    _, B, C = abc(t)
    W = skew(w)
    return EYE + B * W + C * (W * W)


def pose_exp(xi):
    return Exp(xi[:3]), V(xi[:3]) * vec(xi[3:])


def pose_log(R, t):
    """[omega; u] of an exact pose: u = V(omega)^-1 t"""
    w = Log(R)
    u = t if norm(w) == 0 else mp.lu_solve(V(w), t)
    return tuple(w) + tuple(u)


def compose(a, b):
    return a[0] * b[0], a[0] * b[1] + a[1]


def inverse(a):
    return a[0].T, -(a[0].T * a[1])


def between(a, b):
    """a^-1 b with the rotation taken to its nearest rotation (see the module docstring)"""
    return rel(a[0], b[0]), a[0].T * (b[1] - a[1])


def error(mode, des, T):
    """the workspace factor's error of the link pose T against des: mode 1 Log of the rotation, mode 2 Log of the pose"""
    Rr, tr = between(des, T)
    return Log(Rr) if mode == 1 else pose_log(Rr, tr)


def error_jacobian(mode, des, T):
    """d error(des, T * Exp(delta)) / d delta at 0, [3|6][6], differenced.  One coordinate of delta moves at a time, so
    Exp(delta) is (Exp(omega), 0) or (I, u) exactly."""
    cols = []
    for j in range(6):
        if mode == 1 and j >= 3:          # the rotation's Log does not see the translation at all
            cols.append([mpf(0)] * 3)
            continue
        out = []
        for sgn in (1, -1):
            d = [sgn * STEP if k == j else mpf(0) for k in range(6)]
            moved = compose(T, (Exp(d[:3]), vec(d[3:])))
            # T's rotation is not exactly one either; rel() takes the nearest rotation of the product, as at delta = 0
            out.append(error(mode, des, moved))
        cols.append([(p - m) / (2 * STEP) for p, m in zip(*out)])
    return [[cols[j][r] for j in range(6)] for r in range(len(cols[0]))]


def adjoint(T):
    """Ad of a pose in the order [omega; v]: [[R, 0], [[t]x R, R]]"""
    R, t = T
    S = skew(t) * R
    A = mp.zeros(6)
    for i in range(3):
        for j in range(3):
            A[i, j] = A[i + 3, j + 3] = R[i, j]
            A[i + 3, j] = S[i, j]
    return A


# ------------------------------------------------------------------------------------------------ forward kinematics
def _rz(th):
    c, s = mp.cos_sin(th)
    return mp.matrix([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def _fk(fk_model, q):
    """[(pose of link l, J6 [6][D])]: the frames each coordinate of q moves in, with its body twist there; the DH
    chain of an Arm is H_i = Rz(q_i + bias_i) Trans(0, 0, d_i) Trans(a_i, 0, 0) Rx(alpha_i), so joint i turns about z of
    the frame before it; a Pose2 base moves by (dx, dy, dtheta) composed on the right, twists e_vx, e_vy, e_wz of its
    own frame.  J6 column = Ad(link^-1 frame) twist: the body Jacobian in the convention of k_fk."""
    from gpmp2_amd import robots
    q = tuple(v if isinstance(v, mpf) else mpf(float(v)) for v in q)      # doubles, or mpf (the q-difference of the test)
    frames, links = [], []          # (frame pose, twist index 0..5) per coordinate; link poses with the coordinates before
    if isinstance(fk_model, robots.Pose2MobileArm):
        veh = (_rz(q[2]), vec([q[0], q[1], 0]))
        frames += [(veh, 3), (veh, 4), (veh, 2)]
        links.append((veh, 3))
        arm, cur, q = fk_model.arm, compose(veh, pose_of(fk_model.base_T_arm)), q[3:]
    else:
        arm, cur = fk_model, None
    cur = compose(cur, pose_of(arm.base_pose)) if cur is not None else pose_of(arm.base_pose)
    for i in range(arm.dof()):
        frames.append((cur, 2))
        al = mpf(float(arm.alpha[i]))
        ca, sa = mp.cos_sin(al)
        C = (mp.matrix([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]), vec([mpf(float(arm.a[i])), 0, mpf(float(arm.d[i]))]))
        cur = compose(compose(cur, (_rz(q[i] + mpf(float(arm.theta_bias[i]))), vec([0, 0, 0]))), C)
        links.append((cur, len(frames)))
    D = len(frames)
    out = []
    for T, n in links:
        J = mp.zeros(6, D)
        Tinv = inverse(T)
        for k in range(n):
            A = adjoint(compose(Tinv, frames[k][0]))
            for r in range(6):
                J[r, k] = A[r, frames[k][1]]
        out.append((T, J))
    return out


_FK_CACHE = {}


def fk(fk_model, q, link):
    """(pose, J6) of one link at the doubles q, cached per (model, q)"""
    key = (id(fk_model), tuple(float(v) for v in q))
    if key not in _FK_CACHE:
        _FK_CACHE[key] = _fk(fk_model, q)
    return _FK_CACHE[key][link]


def rounded(T):
    """the pose as the doubles a kernel would be given: 4x4 nested lists"""
    R, t = T
    return [[float(R[i, j]) for j in range(3)] + [float(t[i])] for i in range(3)] + [[0.0, 0.0, 0.0, 1.0]]


def factor(fk_model, link, q, des16, mode, jac=True):
    """(err [3|6], H [3|6][D] or None, scale) of the workspace factor, exact for the doubles q and des16 [4][4]"""
    T, J6 = fk(fk_model, q, link)
    des = pose_of(des16)
    err = error(mode, des, T)
    H = None
    if jac:
        E = mp.matrix(error_jacobian(mode, des, T)) * J6
        H = [[E[r, c] for c in range(E.cols)] for r in range(E.rows)]
    scale = max(1.0, max(abs(float(x)) for x in T[1]), max(abs(float(x)) for x in des[1]))
    return err, H, scale


# ------------------------------------------------------------------------------------------------ the path check
def geodesic_target(des_a, des_b, tau):
    """the target the path check forms between two support targets: Rt Exp(tau Log(Rt^T R1)), position on the chord"""
    a, b = pose_of(des_a), pose_of(des_b)
    tau = mpf(float(tau))
    w = Log(rel(a[0], b[0]))
    return a[0] * Exp([tau * x for x in w]), a[1] + tau * (b[1] - a[1])


def deviation(mode, target, T):
    """(pos_dev, rot_dev, |error|^2) of the link pose T against an exact target (R, t)"""
    Rr = polar(target[0].T * T[0])
    d = T[1] - target[1]
    w = Log(Rr)
    rot = norm(w)
    if mode == 1:
        return mpf(0), rot, rot * rot
    xi = pose_log(Rr, target[0].T * d)
    return norm(d), rot, sum(x * x for x in xi)
