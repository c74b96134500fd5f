"""The cases of the SO(3) / SE(3) map tests: shared by tests/test_lie3_maps_cpu.py, tests/test_gpu_lie3_maps.py and
scripts/lie3_maps_error.py, which all measure through `measure` and `measure_path` below.

A factor case is (robot, link, q, des, mode): des = T_link(q) * (Exp(theta a), t)^-1 formed in mpmath and rounded to
doubles, so that between(des, T_link(q)) is the rotation by theta about a with translation t; everything is then
measured from the doubles q and des (tests/lie3_reference.py).  theta runs through every band of the old and the new
forms, from 0 over 1e-18 to pi - 1e-9, and through every switch of the new forms at 0.99 and 1.01 times its value; the
axes through +-x, +-y, +-z (next to pi these walk the three diagonal entries the axis can be taken from, in both signs)
and two generic ones, one with a component of 1e-8; the translations (pose mode) through O(1), zero, large and small.
Every (theta, axis) is one orientation and one pose case; robot configuration and translation cycle with them.  From
1 rad on every angle meets all eight axes; below, where no form looks at the axis, four of them (the exact reference
costs 35 ms a case).  Six angles meet every translation.  Separate sets: targets at exactly pi, compared on the group;
targets whose rotation block is rounded to float32; the path check (below).

For every case and output group, e = max |got - exact| / scale with scale = max(1, largest |translation coordinate| of
des and of the link pose).  The cost groups of the path set are sums of squares: their scale is max(1, |exact|).
"""
from __future__ import annotations

import functools
import math

import numpy as np

import lie3_reference as ref
from lie3_reference import mp, mpf

PI = math.pi
ORIENTATION, POSE = 1, 2
# every constant at which the code under test switches form (csrc/lie_log.h): theta^2 <= 2.22e-16 in so3_k and
# rot3_expmap, LIE_Q_SERIES_BELOW, and c = cos(theta) = -1/2 in rot3_logmap; each enters at 0.99 and 1.01 times its value
SWITCHES = [math.sqrt(2.220446049250313e-16), 0.25, 2.0 * PI / 3.0]
THETAS = [0.0, 1e-18, 3e-11, 9.9e-11, 1.01e-10, 1e-9, 1.4e-8, 1.6e-8, 1e-7, 1e-6, 9.9e-6, 1.01e-5, 1e-4, 3.1e-4, 3.2e-4,
          1e-3, 1e-2, 0.1, 1.0, 2.0, 3.0, PI - 1e-3, PI - 1e-4, PI - 2e-5, PI - 1.01e-5, PI - 9.9e-6, PI - 1e-6, PI - 1e-9]
for _c in SWITCHES:
    for _f in (0.99, 1.01):
        if not any(abs(_f * _c - m) <= 1e-12 * _c for m in THETAS):
            THETAS.append(_f * _c)
_G1 = np.array([0.48, -0.6, 0.64])                              # a unit vector in doubles to 1e-16
_G2 = np.array([1e-8, 0.6, -0.8])
AXES = [(1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0),
        tuple(_G1 / np.linalg.norm(_G1)), tuple(_G2 / np.linalg.norm(_G2))]
SMALL_ANGLE_AXES = (0, 5, 6, 7)      # below 1 rad the forms do not look at the axis: +x, -z and the generic two
TRANSLATIONS = [(0.7, -0.4, 0.3), (0.0, 0.0, 0.0), (30.0, -20.0, 10.0), (1e-3, 2e-3, -1e-3)]
# (robot, link, q): the WAM's last link at two generic configurations (J6 [6][7] of full row rank: every entry of the
# map's Jacobian shows in H) and a mobile manipulator's last link
CONFIGS = [("wam", 6, (0.3, -0.8, 0.5, 1.1, -0.6, 0.9, -0.4)), ("wam", 6, (-1.2, 0.7, -0.9, 1.7, 0.8, -1.1, 0.6)),
           ("mobile", 2, (0.4, -0.3, 0.7, 0.5, -0.9))]

CAP = 1e-12
FACTOR_GROUPS = ("rot.err", "rot.H", "pose.err", "pose.H")
PATH_GROUPS = ("path.rot_dev", "path.pos_dev", "path.cost")
GROUPS = FACTOR_GROUPS + PATH_GROUPS


@functools.lru_cache(maxsize=None)
def models():
    import gpmp2_amd as g
    return dict(wam=g.generateArm("WAMArm"), mobile=g.generateMobileArm("SimpleTwoLinksArm"))


def handles(impl):
    return {k: impl.robot(m) for k, m in models().items()}


def _des(T, theta, axis, t):
    """T * (Exp(theta axis), t)^-1, rounded to doubles"""
    a = ref.M(axis)
    n = ref.norm(a)
    th = mpf(float(theta))
    off = (ref.Exp([th * x / n for x in a]), ref.vec(ref.M(t)))
    return ref.rounded(ref.compose(T, ref.inverse(off)))


def _link_pose(c):
    name, link, q = CONFIGS[c]
    return ref.fk(models()[name].fk_model(), q, link)[0]


@functools.lru_cache(maxsize=None)
def cases():
    """[(config index, mode, des [4][4], theta, axis index, translation index)]"""
    out = []
    for i, th in enumerate(THETAS):
        for k, ax in enumerate(AXES):
            if (th == 0.0 and k > 0) or (th < 1.0 and k not in SMALL_ANGLE_AXES):
                continue
            c, tr = (i + k) % len(CONFIGS), (i + 3 * k) % len(TRANSLATIONS)
            out.append((c, ORIENTATION, _des(_link_pose(c), th, ax, (0.2, 0.1, -0.3)), th, k, -1))
            out.append((c, POSE, _des(_link_pose(c), th, ax, TRANSLATIONS[tr]), th, k, tr))
    # every translation at the angles where Pose3's log changed form or is hardest: one axis each
    for i, th in enumerate((0.0, 3e-11, 1.01e-10, 1e-4, 1.0, PI - 1e-6)):
        for tr in range(len(TRANSLATIONS)):
            c, k = (i + tr) % len(CONFIGS), (2 * i + tr) % len(AXES)
            out.append((c, POSE, _des(_link_pose(c), th, AXES[k], TRANSLATIONS[tr]), th, k, tr))
    return out


def _err(got, want):
    """max |got - want| of one output against its mpf reference, evaluated in mpf"""
    got, flat = np.asarray(got, dtype=np.float64).reshape(-1), []
    for row in want:
        flat.extend(row) if isinstance(row, (list, tuple)) else flat.append(row)
    assert got.size == len(flat)
    return float(max(abs(mpf(float(g_)) - w_) for g_, w_ in zip(got, flat)))


@functools.lru_cache(maxsize=None)
def reference():
    """[(err, H, scale)] of every case, computed once; asserts that no case sits within 1e-12 of the cut"""
    out = []
    for c, mode, des, _, _, _ in cases():
        name, link, q = CONFIGS[c]
        err, H, scale = ref.factor(models()[name].fk_model(), link, q, des, mode)
        assert PI - float(ref.norm(err[:3])) > 1e-12
        out.append((err, H, scale))
    return out


def _factor(impl, h, case):
    c, mode, des = case[:3]
    name, link, q = CONFIGS[c]
    err, H = impl.workspace_prior_factor(h[name], mode, link, np.array(des), np.array(q)[None])
    return err[0], H[0]


def measure(impl, h):
    """impl: the engine or the oracle, h = handles(impl) -> dict(group -> e [cases of that mode])"""
    e = {g_: [] for g_ in FACTOR_GROUPS}
    for case, (r_err, r_H, scale) in zip(cases(), reference()):
        err, H = _factor(impl, h, case)
        p = "rot" if case[1] == ORIENTATION else "pose"
        e[p + ".err"].append(_err(err, r_err) / scale)
        e[p + ".H"].append(_err(H, r_H) / scale)
    return {k: np.array(v) for k, v in e.items()}


# ------------------------------------------------------------------------------------------------ bands
BANDS = ["theta = 0", "(0, 1e-10)", "[1e-10, 1e-5]", "(1e-5, 1e-2]", "(1e-2, 1]", "(1, pi - 1e-2)",
         "pi - [1e-5, 1e-2]", "pi - (1e-8, 1e-5)", "pi - (0, 1e-8]"]


def band_of(th):
    if th == 0.0:
        return 0
    if PI - th <= 1e-2:
        return 6 if PI - th >= 1e-5 else (7 if PI - th > 1e-8 else 8)
    for k, hi in ((1, 1e-10), (2, 1.0000001e-5), (3, 1.0000001e-2), (4, 1.0)):
        if th < hi or (k == 4 and th == hi):
            return k
    return 5


def case_bands(group):
    if group.startswith("path"):
        return np.array([band_of(max(ch)) for ch in PATH_CHUNKS for _ in PATH_RUNS])
    mode = ORIENTATION if group.startswith("rot") else POSE
    return np.array([band_of(c[3]) for c in cases() if c[1] == mode])


# ------------------------------------------------------------------------------------------------ exactly pi
def _about(a):
    a = np.asarray(a, dtype=np.float64)
    return 2.0 * np.outer(a, a) / (a @ a) - np.eye(3)


@functools.lru_cache(maxsize=None)
def pi_cases():
    """[(config, mode, des, Rrel)] with Rrel = Rd^T Rm, as exactly as doubles allow, diag(-1, -1, 1) and its two
    permutations (Rd is Rm with two columns negated) and the symmetric rotation about a generic axis"""
    out = []
    for n, S in enumerate([np.diag([-1.0, -1.0, 1.0]), np.diag([-1.0, 1.0, -1.0]), np.diag([1.0, -1.0, -1.0]), _about(_G1)]):
        c = n % 2
        T = np.array(ref.rounded(_link_pose(c)))
        des = np.eye(4)
        des[:3, :3] = T[:3, :3] @ S.T
        des[:3, 3] = T[:3, 3] - des[:3, :3] @ np.array([0.2, 0.1, -0.3])
        out.append((c, ORIENTATION if n % 2 == 0 else POSE, des.tolist(), S))
    return out


def measure_pi(impl, h):
    """-> [(| |omega| - pi | in ulps of pi, max |Exp(omega) - nearest rotation of Rd^T Rm|)]: the comparison on the group"""
    out = []
    for c, mode, des, _ in pi_cases():
        err, _ = _factor(impl, h, (c, mode, des))
        w = ref.M(err[:3])
        Rr = ref.rel(ref.pose_of(des)[0], _link_pose(c)[0])
        d = ref.Exp(w) - Rr
        ulps = abs(float(np.linalg.norm(err[:3])) - PI) / math.ulp(PI)
        out.append((ulps, float(max(abs(x) for x in d))))
    return out


# ------------------------------------------------------------------------------------------------ not quite a rotation
NONORTHO_THETAS = [PI - 1e-6, PI - 1e-9, 1e-4, 0.0]


@functools.lru_cache(maxsize=None)
def nonortho_cases():
    """des whose rotation block is the float32 rounding of a rotation: [(config, mode, des, theta)]"""
    out = []
    for n, th in enumerate(NONORTHO_THETAS):
        for mode in (ORIENTATION, POSE):
            c = n % len(CONFIGS)
            des = np.array(_des(_link_pose(c), th, AXES[6], TRANSLATIONS[0]))
            des[:3, :3] = des[:3, :3].astype(np.float32).astype(np.float64)
            out.append((c, mode, des.tolist(), th))
    return out


def measure_nonortho(impl, h):
    """-> [(finite, e of err on the polar factor, e of H on the polar factor)]"""
    out = []
    for case in nonortho_cases():
        c, mode, des, _ = case
        name, link, q = CONFIGS[c]
        err, H = _factor(impl, h, case)
        r_err, r_H, scale = ref.factor(models()[name].fk_model(), link, q, des, mode)
        ok = bool(np.isfinite(err).all() and np.isfinite(H).all())
        out.append((ok, _err(err, r_err) / scale if ok else np.inf, _err(H, r_H) / scale if ok else np.inf))
    return out


# ------------------------------------------------------------------------------------------------ the path check
# the path set: constant trajectories (every state the same configuration, zero velocity: the interpolated
# configuration is the same to rounding, which is inside FLOOR) of the WAM's last link against targets whose
# consecutive relative rotations run through a chunk of THETAS about three generic axes in turn
PATH_N = 12
PATH_DT = 0.5
PATH_SIGMA = 1.0
PATH_LINK = 6
PATH_Q = [CONFIGS[0][2], CONFIGS[1][2], (0.9, 0.4, -0.3, 0.8, 1.2, -0.5, 0.2)]
PATH_AXES = [AXES[6], AXES[7], (0.6, 0.0, 0.8)]
PATH_RUNS = [(1, ORIENTATION), (3, POSE)]              # (inter_step, mode)
_TH = sorted(THETAS)
PATH_CHUNKS = [_TH[k::3][:PATH_N] for k in range(3)]    # interleaved: every chunk holds small, middle and near-pi angles
assert sorted(sum(PATH_CHUNKS, [])) == _TH


@functools.lru_cache(maxsize=None)
def path_targets(chunk):
    """des [N+1][4][4] doubles: des[0] a generic offset from the first row's link pose, des[i+1] = des[i] * (Exp, t)"""
    T = ref.fk(models()["wam"].fk_model(), PATH_Q[0], PATH_LINK)[0]
    cur = ref.compose(T, (ref.Exp(ref.M((0.3, -0.2, 0.4))), ref.vec(ref.M((0.05, -0.1, 0.08)))))
    des = [ref.rounded(cur)]
    ths = list(PATH_CHUNKS[chunk]) + [0.5] * (PATH_N - len(PATH_CHUNKS[chunk]))
    for i, th in enumerate(ths):
        a = ref.M(PATH_AXES[i % 3])
        step = (ref.Exp([mpf(float(th)) * x for x in a]), ref.vec(ref.M((0.02, -0.01, 0.015))))
        cur = ref.compose(ref.pose_of(des[-1]), step)
        des.append(ref.rounded(cur))
    return np.array(des)


@functools.lru_cache(maxsize=None)
def path_reference():
    """{(chunk, run): dict(rot_dev, pos_dev, support_cost, dense_cost [B])}: exact for the doubles des and q"""
    fkm = models()["wam"].fk_model()
    out = {}
    for ch in range(len(PATH_CHUNKS)):
        des = path_targets(ch)
        for r, (J, mode) in enumerate(PATH_RUNS):
            targets = []
            for i in range(PATH_N + 1):
                targets.append(ref.pose_of(des[i]))
                if i < PATH_N:
                    targets += [ref.geodesic_target(des[i], des[i + 1], float(j) / float(J + 1)) for j in range(1, J + 1)]
            rows = []
            for q in PATH_Q:
                T = ref.fk(fkm, q, PATH_LINK)[0]
                dev = [ref.deviation(mode, t, T) for t in targets]
                assert all(PI - float(d[1]) > 1e-3 for d in dev), "a checked state next to the cut"
                sig2 = mpf(PATH_SIGMA) ** 2
                rows.append((max(d[1] for d in dev), max(d[0] for d in dev), sum(d[2] for d in dev[::J + 1]) / sig2,
                             sum(d[2] for d in dev) / sig2))
            out[(ch, r)] = rows
    return out


def path_score(impl, h, mode, des, inter_step, traj):
    """the six outputs of the path check from the engine, or from the oracle's restatement (tests/path_reference.py)"""
    sigma = np.full(PATH_N + 1, PATH_SIGMA)
    if hasattr(impl, "path_score_traj"):
        return impl.path_score_traj(h["wam"], mode, PATH_LINK, des, sigma, PATH_DT, inter_step, traj)
    import path_reference as pr
    return pr.oracle_path_score(impl, models()["wam"], h["wam"], mode, PATH_LINK, des, sigma, PATH_DT, inter_step, traj)


def measure_path(impl, h):
    """-> dict(group -> e [chunks x runs]), the largest over the rows of a call"""
    e = {g_: [] for g_ in PATH_GROUPS}
    rf = path_reference()
    D = len(PATH_Q[0])
    traj = np.zeros((len(PATH_Q), PATH_N + 1, 2 * D))
    traj[:, :, :D] = np.array(PATH_Q)[:, None, :]
    for ch in range(len(PATH_CHUNKS)):
        des = path_targets(ch)
        for r, (J, mode) in enumerate(PATH_RUNS):
            got = path_score(impl, h, mode, des, J, traj)
            assert not np.asarray(got["invalid"]).any()
            rot = pos = cost = 0.0
            for b, (r_rot, r_pos, r_sup, r_dense) in enumerate(rf[(ch, r)]):
                rot = max(rot, float(abs(mpf(float(got["max_rot_dev"][b])) - r_rot)))
                pos = max(pos, float(abs(mpf(float(got["max_pos_dev"][b])) - r_pos)))   # offsets below 1: scale 1
                for k, want in (("support_cost", r_sup), ("dense_cost", r_dense)):
                    cost = max(cost, float(abs(mpf(float(got[k][b])) - want) / max(mpf(1), want)))
            e["path.rot_dev"].append(rot)
            e["path.pos_dev"].append(pos)
            e["path.cost"].append(cost)
    return {k: np.array(v) for k, v in e.items()}
