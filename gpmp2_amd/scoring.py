"""The score-and-select stage in numpy terms: the selection rules of include/gpmp2mi.h ("scoring" and the stages after
it) stated once, and the shape checks of the wrappers in checks.py and plan.py.  The per-row outputs of every stage are
the table of stages.py.  The scores themselves come from the device (k_score); nothing here computes a collision cost."""
from __future__ import annotations

import numpy as np

from . import stages

TRAJ_NOT_SPD = 3   # GPMP2MI_TRAJ_NOT_SPD


def checked_states(total_step, inter_step):
    """Md: number of states the stage checks for a trajectory of total_step intervals."""
    return int(total_step) * (int(inter_step) + 1) + 1


def eligible(final_error, status, min_clearance, out_of_range, required_clearance=0.0, require_in_range=False,
             min_self_clearance=None, invalid=None, required_self_clearance=0.0):
    """Boolean mask [B] of the rows the rule may choose (status None: all fine; out_of_range None: all in range).
    min_self_clearance / invalid (include/gpmp2mi.h "self-collision check"): the row must also keep
    required_self_clearance from itself and have no invalid pair; None: not asked."""
    fe = np.asarray(final_error, dtype=np.float64).reshape(-1)
    clr = np.asarray(min_clearance, dtype=np.float64).reshape(-1)
    ok = np.isfinite(fe)
    if status is not None:
        ok &= np.asarray(status).reshape(-1) != TRAJ_NOT_SPD
    with np.errstate(invalid="ignore"):
        ok &= clr >= required_clearance          # False for a NaN clearance
    if require_in_range and out_of_range is not None:
        ok &= np.asarray(out_of_range).reshape(-1) == 0
    _at_least(ok, min_self_clearance, required_self_clearance)
    _none_set(ok, invalid)
    return ok


def select_rule(final_error, status, min_clearance, out_of_range, required_clearance=0.0, require_in_range=False,
                min_self_clearance=None, invalid=None, required_self_clearance=0.0):
    """(best, n_eligible): the eligible row with the smallest final_error, the lowest row on ties; (-1, 0) if none."""
    ok = eligible(final_error, status, min_clearance, out_of_range, required_clearance, require_in_range,
                  min_self_clearance, invalid, required_self_clearance)
    return pick(final_error, ok)


def pick(final_error, ok):
    """(best, n_eligible) of the mask `ok` [B]: the row with the smallest final_error, the lowest row on ties."""
    fe = np.asarray(final_error, dtype=np.float64).reshape(-1)
    rows = np.flatnonzero(ok)
    if rows.size == 0:
        return -1, 0
    return int(rows[np.argmin(fe[rows])]), int(rows.size)   # argmin returns the first of equal minima


def _none_set(ok, flags):
    """ok &= no flag set (flags None: not asked)"""
    if flags is not None:
        ok &= np.asarray(flags).reshape(-1) == 0


def _at_least(ok, x, bound):
    """ok &= x >= bound (x None: not asked); False for a NaN"""
    if x is not None:
        with np.errstate(invalid="ignore"):
            ok &= np.asarray(x, dtype=np.float64).reshape(-1) >= bound


def _at_most(ok, x, bound):
    """ok &= x <= bound (x None: not asked); False for a NaN"""
    if x is not None:
        with np.errstate(invalid="ignore"):
            ok &= np.asarray(x, dtype=np.float64).reshape(-1) <= bound


def _motion_eligible(base, motion_invalid, pos_margin, required_pos_margin):
    """The mask of `eligible` (its arguments: base) with the motion conditions the three motion-based rules share: no
    non-finite motion quantity and pos_margin >= required_pos_margin (each None: not asked)."""
    ok = eligible(*base)
    _none_set(ok, motion_invalid)
    _at_least(ok, pos_margin, required_pos_margin)
    return ok


def select_inputs(final_error, status, min_clearance, out_of_range, require_in_range):
    """The four arrays of a select_best call as contiguous float64 / int32 [B]; ValueError unless their lengths agree."""
    fe = np.ascontiguousarray(final_error, dtype=np.float64).reshape(-1)
    clr = np.ascontiguousarray(min_clearance, dtype=np.float64).reshape(-1)
    st = None if status is None else np.ascontiguousarray(status, dtype=np.int32).reshape(-1)
    oor = None if out_of_range is None else np.ascontiguousarray(out_of_range, dtype=np.int32).reshape(-1)
    B = fe.size
    for name, x in (("min_clearance", clr), ("status", st), ("out_of_range", oor)):
        if x is not None and x.size != B:
            raise ValueError(f"{name}: expected [{B}] like final_error, got [{x.size}]")
    if require_in_range and oor is None:
        raise ValueError("require_in_range needs out_of_range")
    return B, fe, st, clr, oor


def traj_rows(traj, D, total_step=None):
    """traj as contiguous float64 [B][N+1][2D] (a single [N+1][2D] trajectory becomes B = 1); ValueError otherwise."""
    t = np.ascontiguousarray(traj, dtype=np.float64)
    if t.ndim == 2:
        t = t[None]
    if t.ndim != 3 or t.shape[2] != 2 * D or t.shape[1] < 2 or (total_step is not None and t.shape[1] != total_step + 1):
        n = "N+1" if total_step is None else str(total_step + 1)
        raise ValueError(f"traj: expected [B][{n}][{2 * D}], got {list(np.shape(traj))}")
    return t


SCORE_NAMES, SELF_NAMES = stages.names(stages.SCORE), stages.names(stages.SELF)


def pair_table(data, S=None):
    """A pair table as contiguous float64 [P][4] (sphere A, sphere B, epsilon, sigma); [P][2] / [P][3] rows are completed
    with epsilon 0, sigma 1.  ValueError for another shape, or (S given) ids that are not distinct integers in [0, S)."""
    t = np.asarray(data, dtype=np.float64)
    if t.size == 0:
        return np.zeros((0, 4))
    if t.ndim != 2 or t.shape[1] not in (2, 3, 4):
        raise ValueError(f"pair table: expected [P][4], got {list(t.shape)}")
    full = np.zeros((t.shape[0], 4))
    full[:, 3] = 1.0
    full[:, :t.shape[1]] = t
    ids = full[:, :2]
    if S is not None and not ((ids == np.floor(ids)).all() and (ids >= 0).all() and (ids < S).all()
                              and (ids[:, 0] != ids[:, 1]).all()):
        raise ValueError(f"pair table: sphere ids must be distinct integers in [0, {S})")
    return np.ascontiguousarray(full)


# ---- motion limits (include/gpmp2mi.h "motion limits"): the extended rule and the checks of its wrappers
MOTION_NAMES = stages.names(stages.MOTION)


def feasible_rule(final_error, status, min_clearance, out_of_range, required_clearance=0.0, require_in_range=False,
                  min_self_clearance=None, invalid=None, required_self_clearance=0.0, pos_margin=None, time_scale=None,
                  motion_invalid=None, required_pos_margin=0.0, max_time_scale=np.inf):
    """(best, n_eligible) by the rule of select_rule with three more conditions: no non-finite motion quantity,
    pos_margin >= required_pos_margin, time_scale <= max_time_scale (each None: not asked)."""
    base = (final_error, status, min_clearance, out_of_range, required_clearance, require_in_range, min_self_clearance,
            invalid, required_self_clearance)
    ok = _motion_eligible(base, motion_invalid, pos_margin, required_pos_margin)
    _at_most(ok, time_scale, max_time_scale)
    return pick(final_error, ok)


def motion_limits(D, pos_down=None, pos_up=None, vel=None, acc=None, point_speed=np.inf):
    """The limits as the C side takes them: contiguous float64 [D] arrays or None (a scalar is spread over the D
    coordinates), checked as the C side checks them; ValueError otherwise."""
    def vec(name, x):
        if x is None:
            return None
        a = np.asarray(x, dtype=np.float64)
        a = np.full(D, float(a)) if a.ndim == 0 else np.ascontiguousarray(a)
        if a.shape != (D,) or np.isnan(a).any():
            raise ValueError(f"{name}: expected [{D}] values that are not NaN, got {list(np.shape(x))}")
        return a
    lo, hi, v, a = vec("pos_down", pos_down), vec("pos_up", pos_up), vec("vel", vel), vec("acc", acc)
    if (lo is None) != (hi is None):
        raise ValueError("pos_down and pos_up are given together or not at all")
    if lo is not None and (lo > hi).any():
        raise ValueError("pos_down > pos_up")
    for name, x in (("vel", v), ("acc", a)):
        if x is not None and not (x > 0).all():
            raise ValueError(f"{name}: entries must be > 0")
    point_speed = float(point_speed)
    if not point_speed > 0:
        raise ValueError("point_speed must be > 0 (inf: no limit)")
    return lo, hi, v, a, point_speed


def motion_outputs(B, out=None):
    """The seven per-row outputs of a motion-score call: fresh arrays, or the caller's (checked by stages.outputs)."""
    return stages.outputs(stages.MOTION, B, out=out)


def feasible_thresholds(required_pos_margin, max_time_scale):
    required_pos_margin, max_time_scale = float(required_pos_margin), float(max_time_scale)
    if np.isnan(required_pos_margin) or np.isnan(max_time_scale):
        raise ValueError("required_pos_margin / max_time_scale must not be NaN")
    return required_pos_margin, max_time_scale


# ---- re-timing (include/gpmp2mi.h "re-timing"): the status values, the outputs, the rates and the rule of its selection
RETIME_OK, RETIME_BOUNDARY, RETIME_EMPTY, RETIME_INVALID = range(4)
RETIME_NAMES = stages.names(stages.RETIME)


def retime_outputs(B, Md, D=None, out=None):
    """The per-row outputs of a re-timing call: fresh arrays, or the caller's (checked by stages.outputs).
    D = None: the path form, which has no dense_retimed."""
    return stages.outputs(stages.RETIME, B, Md, D, out, absent=("dense_retimed",) if D is None else ())


def retime_rates(max_rate=1.0, rate_start=None, rate_end=None):
    """(max_rate, rate_start, rate_end) as the C side takes them: None = a free end = -1; ValueError for a NaN, a
    max_rate that is not finite and > 0, or a negative forced rate."""
    max_rate = float(max_rate)
    if not (np.isfinite(max_rate) and max_rate > 0):
        raise ValueError("max_rate must be finite and > 0")
    ends = []
    for name, r in (("rate_start", rate_start), ("rate_end", rate_end)):
        if r is not None and not float(r) >= 0:
            raise ValueError(f"{name} must be >= 0 (None: free)")
        ends.append(-1.0 if r is None else float(r))
    return max_rate, ends[0], ends[1]


def retimed_rule(final_error, status, min_clearance, out_of_range, required_clearance=0.0, require_in_range=False,
                 min_self_clearance=None, invalid=None, required_self_clearance=0.0, pos_margin=None,
                 motion_invalid=None, required_pos_margin=0.0, retime_status=None, duration=None, max_duration=np.inf):
    """(best, n_eligible) by feasible_rule without its time_scale test, and then status == RETIME_OK and
    duration <= max_duration."""
    base = (final_error, status, min_clearance, out_of_range, required_clearance, require_in_range, min_self_clearance,
            invalid, required_self_clearance)
    ok = _motion_eligible(base, motion_invalid, pos_margin, required_pos_margin)
    ok &= np.asarray(retime_status).reshape(-1) == RETIME_OK
    with np.errstate(invalid="ignore"):
        ok &= np.asarray(duration, dtype=np.float64).reshape(-1) <= max_duration
    return pick(final_error, ok)


def retimed_thresholds(required_pos_margin, max_duration):
    required_pos_margin, max_duration = float(required_pos_margin), float(max_duration)
    if np.isnan(required_pos_margin) or np.isnan(max_duration):
        raise ValueError("required_pos_margin / max_duration must not be NaN")
    return required_pos_margin, max_duration


# ---- torque limits (include/gpmp2mi.h "torque limits"): the inertial table, the outputs and the rule of its selection
TORQUE_NAMES = stages.names(stages.TORQUE)
TORQUE_MAX_JOINTS = 8       # k_torque is instantiated for fixed-base arms of 1..8 joints


def dynamics_table(L, dof, mass, com, inertia, gravity=(0.0, 0.0, -9.81), torque=None):
    """The description of gpmp2mi_dynamics_create as the C side takes it: contiguous float64 mass [L], com [L][3],
    inertia [L][6] (ixx iyy izz ixy ixz iyz), gravity [3], torque [dof] or None (a scalar is spread over the joints),
    checked as the C side checks them; ValueError otherwise."""
    def arr(name, x, shape):
        a = np.ascontiguousarray(x, dtype=np.float64)
        if a.shape != shape:
            raise ValueError(f"{name}: expected {list(shape)}, got {list(a.shape)}")
        if not np.isfinite(a).all():
            raise ValueError(f"{name}: every entry must be finite")
        return a
    m, c, i, g = arr("mass", mass, (L,)), arr("com", com, (L, 3)), arr("inertia", inertia, (L, 6)), arr("gravity", gravity, (3,))
    if (m < 0).any():
        raise ValueError("mass: entries must be >= 0")
    if (i[:, :3] < 0).any():
        raise ValueError("inertia: the diagonal entries must be >= 0")
    t = None
    if torque is not None:
        t = np.asarray(torque, dtype=np.float64)
        t = np.full(dof, float(t)) if t.ndim == 0 else np.ascontiguousarray(t)
        if t.shape != (dof,) or not (t > 0).all():          # False for NaN
            raise ValueError(f"torque: expected [{dof}] limits > 0 (inf: none), got {list(np.shape(torque))}")
    return m, c, i, g, t


def torque_outputs(B, Md, D, out=None, tau=True):
    """The per-row outputs of a torque-score call: fresh arrays, or the caller's (checked by stages.outputs).
    tau = False: no [B][Md][D] torques unless the caller brings the array."""
    return stages.outputs(stages.TORQUE, B, Md, D, out, absent=() if tau else ("tau",))


def dynamic_rule(final_error, status, min_clearance, out_of_range, required_clearance=0.0, require_in_range=False,
                 min_self_clearance=None, invalid=None, required_self_clearance=0.0, pos_margin=None, time_scale=None,
                 motion_invalid=None, required_pos_margin=0.0, max_time_scale=np.inf, torque_time_scale=None,
                 torque_invalid=None):
    """(best, n_eligible) by feasible_rule with max(time_scale, torque_time_scale) <= max_time_scale in place of its
    time-scale test, and no non-finite torque.  The maximum starts from 0, and is tested even when neither scale is given."""
    base = (final_error, status, min_clearance, out_of_range, required_clearance, require_in_range, min_self_clearance,
            invalid, required_self_clearance)
    ok = _motion_eligible(base, motion_invalid, pos_margin, required_pos_margin)
    _none_set(ok, torque_invalid)
    scale = np.zeros(ok.size)
    with np.errstate(invalid="ignore"):
        for s in (time_scale, torque_time_scale):
            if s is not None:
                scale = np.maximum(scale, np.asarray(s, dtype=np.float64).reshape(-1))
    _at_most(ok, scale, max_time_scale)
    return pick(final_error, ok)


# ---- re-timing under torque limits (include/gpmp2mi.h): the extra status, the outputs, the affine rows and the rule
RETIME_STATIC = 4
RETIME_DYNAMIC_NAMES = stages.names(stages.RETIME_DYNAMIC)
RETIME_MAX_AFFINE = 8       # affine rows per state of gpmp2mi_retime_path_affine


def retime_affine_outputs(B, Md, out=None):
    """The per-row outputs of the path form: those of re-timing with achieved [B][6]."""
    return stages.outputs(stages.RETIME_AFFINE, B, Md, None, out)


def retime_dynamic_outputs(B, Md, D, out=None, tau=True, coef=True):
    """The per-row outputs of a trajectory or plan call: fresh arrays, or the caller's (checked by stages.outputs).
    tau / coef = False: no tau_retimed [B][Md][D] / coef [B][Md][4][D] unless the caller brings the array."""
    absent = (() if tau else ("tau_retimed",)) + (() if coef else ("coef",))
    return stages.outputs(stages.RETIME_DYNAMIC, B, Md, D, out, absent=absent)


def affine_rows(B, Md, cx_left, cx_right, cu, off, bound):
    """The R affine rows |cx x + cu u + off| <= bound of the path form as the C side takes them: (R, cx_left, cx_right,
    cu, off contiguous float64 [B][Md][R], bound [R]); ValueError for R outside 0..8, a shape that does not fit or a bound
    that is NaN or <= 0 (inf: none)."""
    b = np.ascontiguousarray([] if bound is None else bound, dtype=np.float64).reshape(-1)
    R = b.shape[0]
    if R > RETIME_MAX_AFFINE:
        raise ValueError(f"at most {RETIME_MAX_AFFINE} affine rows per state, got {R}")
    if not (b > 0).all():          # False for NaN
        raise ValueError("bound: every entry must be > 0 (inf: none)")
    rows = []
    for name, x in (("cx_left", cx_left), ("cx_right", cx_right), ("cu", cu), ("off", off)):
        a = np.ascontiguousarray(np.zeros((B, Md, 0)) if x is None else x, dtype=np.float64)
        if a.size != B * Md * R:
            raise ValueError(f"{name}: expected [{B}][{Md}][{R}], got {list(a.shape)}")
        rows.append(a.reshape(B, Md, R))
    return (R, *rows, b)


def retimed_dynamic_rule(*args, coef_finite=None, **kw):
    """(best, n_eligible) by retimed_rule on the profile under torque limits, and no coefficient of the row that is not
    finite (coef_finite: bool [B])."""
    if coef_finite is None:
        return retimed_rule(*args, **kw)
    status = np.where(np.asarray(coef_finite, dtype=bool).reshape(-1), np.asarray(kw["retime_status"]).reshape(-1), -1)
    return retimed_rule(*args, **dict(kw, retime_status=status))


# ---- moving obstacles (include/gpmp2mi.h "moving obstacles"): the output names, the extended rule, the sphere set
MOVING_NAMES = stages.names(stages.MOVING)
MAX_MOVING_SPHERES = 64     # GPMP2MI_MAX_MOVING_SPHERES


def moving_rule(final_error, status, min_clearance, out_of_range, required_clearance=0.0, require_in_range=False,
                min_self_clearance=None, invalid=None, required_self_clearance=0.0, min_moving_clearance=None,
                moving_invalid=None, required_moving_clearance=-np.inf):
    """(best, n_eligible) by the rule of select_rule with two more conditions: no invalid (state, sphere, moving sphere)
    and min_moving_clearance >= required_moving_clearance (each None: not asked)."""
    ok = eligible(final_error, status, min_clearance, out_of_range, required_clearance, require_in_range,
                  min_self_clearance, invalid, required_self_clearance)
    _none_set(ok, moving_invalid)
    _at_least(ok, min_moving_clearance, required_moving_clearance)
    return pick(final_error, ok)


def moving_set(radius, centers, states, capacity=MAX_MOVING_SPHERES):
    """A sphere set as contiguous float64 (radius [K], centers [K][states][3]); None / empty: K = 0.  ValueError for
    another shape or more than `capacity` spheres."""
    r = np.zeros(0) if radius is None else np.ascontiguousarray(radius, dtype=np.float64).reshape(-1)
    K = r.size
    c = np.zeros((0, states, 3)) if centers is None or K == 0 else np.ascontiguousarray(centers, dtype=np.float64)
    if c.shape != (K, states, 3):
        raise ValueError(f"centers: expected [{K}][{states}][3], got {list(c.shape)}")
    if K > capacity:
        raise ValueError(f"{K} moving spheres, room for {capacity}")
    return K, r, c


# ---- carried object (include/gpmp2mi.h "carried object"): the output names, the extended rule, the sphere set
CARRIED_NAMES = stages.names(stages.CARRIED)
MAX_CARRIED_SPHERES = 256   # GPMP2MI_MAX_CARRIED_SPHERES


def carried_rule(final_error, status, min_clearance, out_of_range, required_clearance=0.0, require_in_range=False,
                 min_self_clearance=None, invalid=None, required_self_clearance=0.0, min_carried_clearance=None,
                 carried_out_of_range=None, required_carried_clearance=-np.inf):
    """(best, n_eligible) by the rule of select_rule with two more conditions: no carried sphere out of range when
    require_in_range, and min_carried_clearance >= required_carried_clearance (each None: not asked)."""
    ok = eligible(final_error, status, min_clearance, out_of_range, required_clearance, require_in_range,
                  min_self_clearance, invalid, required_self_clearance)
    if require_in_range:
        _none_set(ok, carried_out_of_range)
    _at_least(ok, min_carried_clearance, required_carried_clearance)
    return pick(final_error, ok)


def carried_set(radius, centers, capacity=MAX_CARRIED_SPHERES):
    """A carried set as contiguous float64 (radius [A], centers [A][3]); None / empty: A = 0.  ValueError for another
    shape or more than `capacity` spheres."""
    r = np.zeros(0) if radius is None else np.ascontiguousarray(radius, dtype=np.float64).reshape(-1)
    A = r.size
    c = np.zeros((0, 3)) if centers is None or A == 0 else np.ascontiguousarray(centers, dtype=np.float64)
    if c.shape != (A, 3):
        raise ValueError(f"centers: expected [{A}][3], got {list(c.shape)}")
    if A > capacity:
        raise ValueError(f"{A} carried spheres, room for {capacity}")
    return A, r, c


# ---- workspace path (include/gpmp2mi.h "workspace path"): the output names, the extended rule, a straight-line path
PATH_NAMES = stages.names(stages.PATH)


def path_arrays(des, sigma, states):
    """A path as contiguous float64 (des [states][4][4], sigma [states]); a scalar sigma is repeated.  ValueError for
    another shape."""
    d = np.ascontiguousarray(des, dtype=np.float64)
    if d.shape == (states, 16):
        d = d.reshape(states, 4, 4)
    if d.shape != (states, 4, 4):
        raise ValueError(f"des: expected [{states}][4][4], got {list(d.shape)}")
    if sigma is None:
        raise ValueError("sigma: a path needs one sigma per state (or a scalar)")
    s =np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (states,)) if np.ndim(sigma) == 0
                             else sigma, dtype=np.float64)
    if s.shape != (states,):
        raise ValueError(f"sigma: expected [{states}], got {list(s.shape)}")
    return d, s


def path_rule(final_error, status, min_clearance, out_of_range, required_clearance=0.0, require_in_range=False,
              max_pos_dev=None, max_rot_dev=None, path_invalid=None, max_pos_dev_allowed=np.inf,
              max_rot_dev_allowed=np.inf):
    """(best, n_eligible) by the rule of select_rule with one more condition: no invalid checked state,
    max_pos_dev <= max_pos_dev_allowed and max_rot_dev <= max_rot_dev_allowed (each None: not asked)."""
    ok = eligible(final_error, status, min_clearance, out_of_range, required_clearance, require_in_range)
    _none_set(ok, path_invalid)
    _at_most(ok, max_pos_dev, max_pos_dev_allowed)
    _at_most(ok, max_rot_dev, max_rot_dev_allowed)
    return pick(final_error, ok)


def _rot_log(R):
    """SO(3) logarithm of a rotation matrix, angle in [0, pi)"""
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.linalg.norm(v)
    th = np.arctan2(s, 0.5 * (np.trace(R) - 1.0))
    return v if s < 1e-12 else v * (th / s)


def _rot_exp(w):
    th = np.linalg.norm(w)
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th * th <= 2.220446049250313e-16:
        return np.eye(3) + W
    return np.eye(3) + (np.sin(th) / th) * W + ((1.0 - np.cos(th)) / (th * th)) * (W @ W)


def line_path(pose_a, pose_b, N, s=None):
    """des [N+1][4][4]: positions on the straight line from pose_a to pose_b, orientations on the geodesic between
    them, at the N + 1 support states.  The end poses are pose_a and pose_b themselves.  s [N+1]: where on the line
    each support state is, from s[0] = 0 to s[N] = 1 (default i / N, constant speed; a motion that starts and ends at
    rest wants an eased profile such as 3 u^2 - 2 u^3 of u = i / N)."""
    A, Bm = np.asarray(pose_a, dtype=np.float64).reshape(4, 4), np.asarray(pose_b, dtype=np.float64).reshape(4, 4)
    if int(N) < 1:
        raise ValueError("N must be >= 1")
    s = np.arange(int(N) + 1) / float(N) if s is None else np.asarray(s, dtype=np.float64).reshape(-1)
    if s.shape != (int(N) + 1,) or s[0] != 0.0 or s[-1] != 1.0:
        raise ValueError(f"s: expected [{int(N) + 1}] from 0 to 1")
    w = _rot_log(A[:3, :3].T @ Bm[:3, :3])
    des = np.zeros((int(N) + 1, 4, 4))
    for i in range(int(N) + 1):
        tau = s[i]
        des[i, :3, :3] = A[:3, :3] @ _rot_exp(tau * w)
        des[i, :3, 3] = A[:3, 3] + tau * (Bm[:3, 3] - A[:3, 3])
        des[i, 3, 3] = 1.0
    des[0], des[int(N)] = A, Bm
    return des


# ---- distinct alternatives (include/gpmp2mi.h): the grouping rule in numpy terms and the shape checks of its wrappers
DIST_MAX_STATE, DIST_RMS = 0, 1
MAX_GROUP_ROWS = 8192       # GPMP2MI_MAX_GROUP_ROWS
MAX_ALTERNATIVES = 64       # GPMP2MI_MAX_ALTERNATIVES


def group_rule(dist, score, eligible, radius):
    """The leader rule: (mode [B], leaders [B], sizes [B], n_modes).  A row takes part iff it is eligible (None: all
    are) and its score is finite; the participating rows are visited by ascending score, the lowest row on ties, and
    each joins the first leader, in leader order, with dist[leader][row] <= radius, or becomes the next leader.  A NaN
    distance is never within the radius.  mode is -1 for rows that do not take part; leaders is -1 and sizes 0 beyond
    n_modes."""
    sc = np.asarray(score, dtype=np.float64).reshape(-1)
    B = sc.size
    d = np.asarray(dist, dtype=np.float64).reshape(B, B)
    part = np.isfinite(sc)
    if eligible is not None:
        part &= np.asarray(eligible).reshape(-1) != 0
    mode = np.full(B, -1, dtype=np.int32)
    leaders = np.full(B, -1, dtype=np.int32)
    sizes = np.zeros(B, dtype=np.int32)
    rows = np.flatnonzero(part)
    order = rows[np.argsort(sc[rows], kind="stable")]   # stable: equal scores keep ascending rows
    n = 0
    for b in order:
        with np.errstate(invalid="ignore"):
            near = np.flatnonzero(d[leaders[:n], b] <= radius)
        k = int(near[0]) if near.size else n
        if k == n:
            leaders[n] = b
            n += 1
        mode[b] = k
        sizes[k] += 1
    return mode, leaders, sizes, n


def group_metric(metric):
    """GPMP2MI_DIST_MAX_STATE / GPMP2MI_DIST_RMS from 0 / 1 or "max_state" / "rms"; ValueError otherwise."""
    names = {"max_state": DIST_MAX_STATE, "rms": DIST_RMS}
    m = names.get(metric, metric) if isinstance(metric, str) else metric
    if m not in (DIST_MAX_STATE, DIST_RMS):
        raise ValueError(f"metric: expected 0 / 'max_state' or 1 / 'rms', got {metric!r}")
    return int(m)


def group_weights(weights, D):
    """weights as contiguous float64 [D] of finite values >= 0, or None; ValueError otherwise."""
    if weights is None:
        return None
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (D,) or not (np.isfinite(w).all() and (w >= 0).all()):
        raise ValueError(f"weights: expected [{D}] finite values >= 0, got {list(np.shape(weights))}")
    return w


def group_radius(radius):
    radius = float(radius)
    if not radius >= 0.0:
        raise ValueError("radius must be >= 0")
    return radius


def group_inputs(B, score, eligible, dist=None, limit=True):
    """score float64 [B], eligible int32 [B] or None, dist float64 [B][B] or None, contiguous; ValueError for other
    shapes or, with `limit` (the forms that use the device), B > MAX_GROUP_ROWS."""
    if limit and B > MAX_GROUP_ROWS:
        raise ValueError(f"at most {MAX_GROUP_ROWS} rows can be grouped, got {B}")
    sc = np.ascontiguousarray(score, dtype=np.float64)
    if sc.shape != (B,):
        raise ValueError(f"score: expected [{B}], got {list(sc.shape)}")
    el = None
    if eligible is not None:
        el = np.ascontiguousarray(np.asarray(eligible) != 0, dtype=np.int32)
        if el.shape != (B,):
            raise ValueError(f"eligible: expected [{B}], got {list(el.shape)}")
    if dist is None:
        return sc, el
    d = np.ascontiguousarray(dist, dtype=np.float64)
    if d.shape != (B, B):
        raise ValueError(f"dist: expected [{B}][{B}], got {list(d.shape)}")
    return sc, el, d


def group_outputs(B):
    return dict(mode=np.full(B, -1, dtype=np.int32), leaders=np.full(B, -1, dtype=np.int32),
                sizes=np.zeros(B, dtype=np.int32))
