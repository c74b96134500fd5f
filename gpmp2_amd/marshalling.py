"""What the wrappers of engine.py, checks.py, fields.py and plan.py share in front of a call of the C ABI: the checks of
host inputs, the device arguments of the `_dev` forms, the pointer tuples and argument lists that follow from the table
of check stages (stages.py), the limit and dynamics objects, and the handle that destroys what the library created.
Nothing here loads the library."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi, scoring, stages
from ._capi import dptr, f64, iptr


def seed_inputs(D, N, start_conf, end_conf, mean, M=None):
    """The rows of a seeded call as contiguous float64 arrays: start_conf, end_conf [M][D] (both may be None when a mean
    is given), mean [M][N+1][2D] or None -> (M, start_conf, end_conf, mean); ValueError when they disagree on M."""
    sc = None if start_conf is None else f64(start_conf).reshape(-1, D)
    ec = None if end_conf is None else f64(end_conf).reshape(-1, D)
    mu = None if mean is None else f64(mean).reshape(-1, N + 1, 2 * D)
    if mu is None and (sc is None or ec is None):
        raise ValueError("start_conf and end_conf are required when no mean is given")
    counts = [x.shape[0] for x in (sc, ec, mu) if x is not None] + ([] if M is None else [int(M)])
    if len(set(counts)) != 1 or counts[0] < 1:
        raise ValueError(f"seeded inputs disagree on the number of problems: {counts}")
    return counts[0], sc, ec, mu


def queue_inputs(D, N, start_conf, start_vel, end_conf, end_vel, init):
    """The M problems of a queue run as contiguous float64 arrays ([M][D] x 4, [M][N+1][2D]); ValueError unless every
    input has the same number M >= 1 of rows and the plan's row shape."""
    rows = [f64(x) for x in (start_conf, start_vel, end_conf, end_vel)]
    t = f64(init)
    rows = [x.reshape(1, D) if x.shape == (D,) else x for x in rows]
    if t.shape == (N + 1, 2 * D):
        t = t.reshape(1, N + 1, 2 * D)
    for name, x in zip(("start_conf", "start_vel", "end_conf", "end_vel"), rows):
        if x.ndim != 2 or x.shape[1] != D:
            raise ValueError(f"{name}: expected [M][{D}], got {list(x.shape)}")
    if t.ndim != 3 or t.shape[1:] != (N + 1, 2 * D):
        raise ValueError(f"init: expected [M][{N + 1}][{2 * D}], got {list(t.shape)}")
    M = t.shape[0]
    if M < 1 or any(x.shape[0] != M for x in rows):
        raise ValueError(f"queue inputs disagree on the number of problems: {[x.shape[0] for x in rows] + [M]}")
    return M, rows, t


def _dev_arg(name, x, shape, integer=False):
    """A device output of a `_dev` call as c_void_p: None, a raw device pointer (int), or a torch tensor checked for
    device, dtype, contiguity and shape."""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        want = "torch.int32" if integer else "torch.float64"
        if str(x.dtype) != want or not x.is_contiguous() or tuple(x.shape) != tuple(shape) or x.device.type != "cuda":
            raise ValueError(f"{name}: expected a contiguous {want} cuda tensor of shape {list(shape)}, got "
                             f"{x.dtype} {list(x.shape)} on {x.device}")
        x = x.data_ptr()
    return C.c_void_p(int(x))


def _score_args(inter_step):
    inter_step = int(inter_step)
    if inter_step < 0:
        raise ValueError("inter_step must be >= 0")
    return inter_step


def traj_args(traj, dof, delta_t, inter_step):
    """The head of a check of host trajectories: (traj as contiguous [B][N+1][2 dof], inter_step, delta_t, B, N), checked."""
    t = scoring.traj_rows(traj, dof)
    inter_step = _score_args(inter_step)
    if not float(delta_t) > 0:
        raise ValueError("delta_t must be > 0")
    return t, inter_step, float(delta_t), t.shape[0], t.shape[1] - 1


def out_ptrs(stage, o):
    """The trailing pointers of a host call of `stage` (stages.py), in C argument order, from the dict o of
    stages.outputs; an output the call goes without is NULL or not there, as the dict has it."""
    return [(iptr if dt is np.int32 else dptr)(o[name]) for name, dt, _ in stage.outputs if name in o]


def dev_args(stage, B, Md, D, given):
    """The trailing device outputs of a `_dev` call of `stage`, in C argument order: given[name] is the caller's buffer
    for the output of that name (a method passes its locals()), each through _dev_arg with the table's shape."""
    return [_dev_arg(name, given[name], shape, dt is np.int32) for name, dt, shape in stages.shapes(stage, B, Md, D)]


class MotionLimits:
    """gpmp2mi_motion_limits for a robot of `dof` coordinates (include/gpmp2mi.h "motion limits"): pos_down / pos_up /
    vel / acc are [dof] arrays, scalars (spread over the coordinates) or None = no limit of that kind; infinite entries
    mean no limit for that coordinate; point_speed in m/s, inf = none.  Validated as the C side validates
    (ValueError); the arrays live as long as this object."""

    def __init__(self, dof, pos_down=None, pos_up=None, vel=None, acc=None, point_speed=np.inf):
        self.dof = int(dof)
        self.pos_down, self.pos_up, self.vel, self.acc, self.point_speed = scoring.motion_limits(
            self.dof, pos_down, pos_up, vel, acc, point_speed)
        self.c = _capi.MotionLimitsC(dptr(self.pos_down), dptr(self.pos_up), dptr(self.vel), dptr(self.acc),
                                     self.point_speed)

    def ref(self, dof):
        if dof != self.dof:
            raise ValueError(f"these limits are for dof {self.dof}, not {dof}")
        return C.byref(self.c)


def _limits_arg(limits, dof):
    """limits: a MotionLimits, or None = no limit at all"""
    return (limits if limits is not None else MotionLimits(dof)).ref(dof)


class Dynamics:
    """gpmp2mi_dynamics for `robot` (include/gpmp2mi.h "torque limits"): the inertial table of a fixed-base arm on the
    device, bound to the robot's kinematics.  mass [L], com [L][3] in the link frames, inertia [L][6] = ixx iyy izz ixy
    ixz iyz about the centres of mass, gravity [3] in the world frame, torque [dof] limits (a scalar is spread over the
    joints; inf: none for that joint) or None = no limit.  Validated as the C side validates (ValueError) before the
    library is called."""

    def __init__(self, eng, robot, mass, com, inertia, gravity=(0.0, 0.0, -9.81), torque=None):
        self.L, self.dof = int(robot.L), int(robot.dof)
        self.mass, self.com, self.inertia, self.gravity, self.torque = scoring.dynamics_table(
            self.L, self.dof, mass, com, inertia, gravity, torque)
        desc = _capi.DynamicsDescC(dptr(self.mass), dptr(self.com), dptr(self.inertia), (C.c_double * 3)(*self.gravity),
                                   dptr(self.torque))
        out = C.c_void_p()
        eng._ck(eng.lib.gpmp2mi_dynamics_create(robot.ptr, C.byref(desc), C.byref(out)))
        self._h = _Handle(out, eng.lib.gpmp2mi_dynamics_destroy)

    @property
    def ptr(self):
        return self._h.ptr

    def close(self):
        self._h.close()


def _kappa_arg(kappa):
    kappa = float(kappa)
    if not (np.isfinite(kappa) and kappa >= 0.0):
        raise ValueError("kappa must be finite and >= 0")
    return kappa


def sampled_args(inter_step, K, row_first, sample_first, required_clearance=0.0):
    """The scalars of a sampled-clearance call, checked: (inter_step, K, row_first, sample_first, required_clearance)."""
    inter_step, K, row_first, sample_first = _score_args(inter_step), int(K), int(row_first), int(sample_first)
    if K < 1:
        raise ValueError("K must be >= 1")
    if row_first < 0 or sample_first < 0:
        raise ValueError("row_first and sample_first must be >= 0")
    required_clearance = float(required_clearance)
    if np.isnan(required_clearance):
        raise ValueError("required_clearance must not be NaN")
    return inter_step, K, row_first, sample_first, required_clearance


def sampled_outputs(B, K, Md, D, want_maps=True, want_conf=False):
    """Fresh host arrays for the outputs of a sampled-clearance call (state_clearance / conf: None unless wanted)."""
    return dict(hits=np.zeros(B, dtype=np.int32), probability=np.zeros(B), clearance=np.zeros((B, K)),
                worst=np.zeros((B, K, 2), dtype=np.int32),
                state_clearance=np.zeros((B, K, Md)) if want_maps else None,
                state_hits=np.zeros((B, Md), dtype=np.int32), oor_samples=np.zeros(B, dtype=np.int32),
                conf=np.zeros((B, K, Md, D)) if want_conf else None)


def _sampled_ptrs(o):
    return (iptr(o["hits"]), dptr(o["probability"]), dptr(o["clearance"]), iptr(o["worst"]), dptr(o["state_clearance"]),
            iptr(o["state_hits"]), iptr(o["oor_samples"]))


def _sampled_dev_args(B, K, Md, hits, probability, clearance, worst, state_clearance, state_hits, oor_samples):
    return [_dev_arg("hits", hits, (B,), True), _dev_arg("probability", probability, (B,)),
            _dev_arg("clearance", clearance, (B, K)), _dev_arg("worst", worst, (B, K, 2), True),
            _dev_arg("state_clearance", state_clearance, (B, K, Md)), _dev_arg("state_hits", state_hits, (B, Md), True),
            _dev_arg("oor_samples", oor_samples, (B,), True)]


def band_inputs(D, Sdiag, Soff, Qc=None):
    """The band of a posterior as contiguous float64 arrays: Sdiag [B][N+1][2D][2D], Soff [B][N][2D][2D] (one row may
    come without the batch axis), Qc [D][D] or None -> (B, N, Sdiag, Soff, Qc); ValueError when the shapes disagree."""
    n = 2 * int(D)
    Sd, So = f64(Sdiag), f64(Soff)
    if Sd.ndim == 3:
        Sd = Sd.reshape((1,) + Sd.shape)
    if So.ndim == 3:
        So = So.reshape((1,) + So.shape)
    if Sd.ndim != 4 or Sd.shape[1] < 2 or Sd.shape[2:] != (n, n):
        raise ValueError(f"Sdiag: expected [B][N+1][{n}][{n}] with N >= 1, got {list(Sd.shape)}")
    B, N = Sd.shape[0], Sd.shape[1] - 1
    if So.shape != (B, N, n, n):
        raise ValueError(f"Soff: expected [{B}][{N}][{n}][{n}], got {list(So.shape)}")
    q = None
    if Qc is not None:
        q = f64(Qc)
        if q.shape != (D, D):
            raise ValueError(f"Qc: expected [{D}][{D}], got {list(q.shape)}")
    return B, N, Sd, So, q


def multi_plan_args(B, devices):
    """(B, devices as a list of ints); ValueError for an empty list, more than MAX_SHARDS devices or B < len(devices)."""
    devices = [int(x) for x in devices]
    if not devices:
        raise ValueError("devices must name at least one device")
    if len(devices) > _capi.MAX_SHARDS:
        raise ValueError(f"at most {_capi.MAX_SHARDS} shards, got {len(devices)}")
    if int(B) < len(devices):
        raise ValueError(f"B = {int(B)} is smaller than the number of shards ({len(devices)})")
    return int(B), devices


class _Handle:
    def __init__(self, ptr, destroy, keep=None):
        self.ptr, self._destroy, self.keep = ptr, destroy, keep

    def close(self):
        if self.ptr:
            self._destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
