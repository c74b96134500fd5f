"""ctypes binding of the HIP product library (gpmp2_amd/csrc/libgpmp2mi.so, C ABI of
include/gpmp2mi.h).  There is no Python/CPU compute path here: if the shared library is missing
or no GPU is usable every call raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _capi, scoring
from ._capi import dptr, f64, iptr

_HERE = os.path.dirname(os.path.abspath(__file__))
# GPMP2MI_LIB: another build of the same library (diagnostic / A-B builds); the default is the in-tree product library
LIB_PATH = os.environ.get("GPMP2MI_LIB") or os.path.join(_HERE, "csrc", "libgpmp2mi.so")

ERR_NAMES = {1: "invalid argument", 2: "no usable GPU", 3: "HIP error", 4: "unsupported", 5: "allocation failed",
             6: "timed out (plan poisoned)"}


# per-trajectory status (include/gpmp2mi.h:51-59)
TRAJ_CONVERGED, TRAJ_MAX_ITER, TRAJ_ROLLED_BACK, TRAJ_NOT_SPD, TRAJ_ALREADY_OPTIMAL = range(5)


class Gpmp2miError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"gpmp2mi error {code} ({ERR_NAMES.get(code, '?')}): {msg}")
        self.code = code


def load_library(path: str = LIB_PATH) -> C.CDLL:
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no fallback implementation)")
    lib = C.CDLL(path)
    lib.gpmp2mi_last_error.restype = C.c_char_p
    lib.gpmp2mi_plan_traj_dev.restype = C.c_void_p
    for name in ("gpmp2mi_robot_destroy", "gpmp2mi_sdf_destroy", "gpmp2mi_plan_destroy"):
        getattr(lib, name).argtypes = [C.c_void_p]
        getattr(lib, name).restype = None
    _capi.declare_queue(lib)
    _capi.declare_multi(lib)
    _capi.declare_score(lib)
    _capi.declare_self(lib)
    _capi.declare_motion(lib)
    _capi.declare_retime(lib)
    _capi.declare_torque(lib)
    _capi.declare_moving(lib)
    _capi.declare_selfpair(lib)
    _capi.declare_path(lib)
    _capi.declare_map(lib)
    _capi.declare_sensor(lib)
    _capi.declare_scene(lib)
    _capi.declare_group(lib)
    _capi.declare_posterior(lib)
    _capi.declare_risk(lib)
    _capi.declare_seed(lib)
    _capi.declare_sampled(lib)
    _capi.declare_ik(lib)
    return lib


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


def _score_ptrs(o):
    return (dptr(o["support_cost"]), dptr(o["dense_cost"]), dptr(o["min_clearance"]), iptr(o["worst"]),
            iptr(o["out_of_range"]))


def _self_ptrs(o):
    return (dptr(o["self_support_cost"]), dptr(o["self_dense_cost"]), dptr(o["min_self_clearance"]), iptr(o["worst"]),
            iptr(o["invalid"]))


def _moving_ptrs(o):
    return (dptr(o["moving_support_cost"]), dptr(o["moving_dense_cost"]), dptr(o["min_moving_clearance"]),
            iptr(o["worst"]), iptr(o["invalid"]))


def _path_ptrs(o):
    return (dptr(o["max_pos_dev"]), dptr(o["max_rot_dev"]), iptr(o["worst"]), dptr(o["support_cost"]),
            dptr(o["dense_cost"]), iptr(o["invalid"]))


def _motion_ptrs(o):
    return (dptr(o["pos_margin"]), dptr(o["vel_ratio"]), dptr(o["acc_ratio"]), dptr(o["point_speed"]),
            dptr(o["time_scale"]), iptr(o["worst"]), iptr(o["invalid"]))


def _torque_ptrs(o):
    return (dptr(o["torque_ratio"]), dptr(o["static_ratio"]), dptr(o["torque_time_scale"]), iptr(o["worst"]),
            iptr(o["invalid"]), dptr(o["tau"]))


def _retime_ptrs(o):
    return (dptr(o["sdot"]), dptr(o["u"]), dptr(o["stamps"]), dptr(o["duration"]), iptr(o["status"]),
            dptr(o["achieved"])) + ((dptr(o["dense_retimed"]),) if "dense_retimed" in o else ())


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


class Engine:
    """Thin object wrapper; method names mirror tests/oracle.py one-to-one."""

    def __init__(self, path: str = LIB_PATH):
        self.lib = load_library(path)

    def _ck(self, rc):
        if rc != 0:
            raise Gpmp2miError(rc, self.lib.gpmp2mi_last_error().decode())

    def device_count(self):
        return int(self.lib.gpmp2mi_device_count())

    # ---------------------------------------------------------------- handles
    def robot(self, model):
        desc, keep = _capi.make_robot_desc(model)
        out = C.c_void_p()
        self._ck(self.lib.gpmp2mi_robot_create(C.byref(desc), C.byref(out)))
        h = _Handle(out, self.lib.gpmp2mi_robot_destroy, keep)
        h.dof, h.S, h.L = model.dof(), model.nr_body_spheres(), model.fk_model().nr_links()
        return h

    def sdf(self, origin, cell_size, data, layout=_capi.SDF_LAYOUT_ZYX):
        data = f64(data)
        dim = data.ndim
        if dim == 2:
            ny, nx, nz = data.shape[0], data.shape[1], 1
        else:
            nz, ny, nx = data.shape
        org = f64(list(origin) + [0.0] * (3 - len(origin)))
        out = C.c_void_p()
        self._ck(self.lib.gpmp2mi_sdf_create(C.c_int(dim), dptr(org), C.c_double(cell_size), nx, ny, nz,
                                             dptr(data), C.c_int(layout), C.byref(out)))
        h = _Handle(out, self.lib.gpmp2mi_sdf_destroy)
        h.dim, h.shape = dim, data.shape
        return h

    def sdf_field_from_occupancy(self, occ, cell_size):
        """occupancy [ny][nx] or [nz][ny][nx] -> signed field of the same shape (computed on the GPU)"""
        occ = f64(occ)
        dim = occ.ndim
        nz, ny, nx = ((1,) + occ.shape) if dim == 2 else occ.shape
        field = np.zeros_like(occ)
        self._ck(self.lib.gpmp2mi_sdf_field_from_occupancy(C.c_int(dim), nx, ny, nz, dptr(occ), C.c_double(cell_size),
                                                           dptr(field)))
        return field

    def sdf_from_occupancy(self, origin, cell_size, occ, layout=_capi.SDF_LAYOUT_ZYX):
        occ = f64(occ)
        dim = occ.ndim
        nz, ny, nx = ((1,) + occ.shape) if dim == 2 else occ.shape
        org = f64(list(origin) + [0.0] * (3 - len(origin)))
        out = C.c_void_p()
        self._ck(self.lib.gpmp2mi_sdf_create_from_occupancy(C.c_int(dim), dptr(org), C.c_double(cell_size), nx, ny, nz,
                                                            dptr(occ), C.c_int(layout), C.byref(out)))
        h = _Handle(out, self.lib.gpmp2mi_sdf_destroy)
        h.dim, h.shape = dim, occ.shape
        return h

    def sdf_read_vol(self, filename_pre):
        out = C.c_void_p()
        self._ck(self.lib.gpmp2mi_sdf_read_vol(str(filename_pre).encode(), C.byref(out)))
        h = _Handle(out, self.lib.gpmp2mi_sdf_destroy)
        h.dim = 3
        return h

    def sdf_field(self, sdf):
        """-> dict(dim, origin, cell_size, data [nz][ny][nx] or [ny][nx])"""
        dim, nx, ny, nz = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        org, cell = np.zeros(3), C.c_double()
        self._ck(self.lib.gpmp2mi_sdf_get_field(sdf.ptr, C.byref(dim), C.byref(nx), C.byref(ny), C.byref(nz), dptr(org),
                                                C.byref(cell), None))
        data = np.zeros((nz.value, ny.value, nx.value))
        self._ck(self.lib.gpmp2mi_sdf_get_field(sdf.ptr, None, None, None, None, None, None, dptr(data)))
        return dict(dim=dim.value, origin=org[:dim.value].copy(), cell_size=cell.value,
                    data=data[0] if dim.value == 2 else data)

    # ---------------------------------------------------------------- factor level
    def sdf_query(self, sdf, points):
        p = f64(points).reshape(-1, sdf.dim)
        M = p.shape[0]
        dist, grad, inr = np.zeros(M), np.zeros((M, sdf.dim)), np.zeros(M, dtype=np.int32)
        self._ck(self.lib.gpmp2mi_sdf_query(sdf.ptr, M, dptr(p), dptr(dist), dptr(grad), iptr(inr)))
        return dist, grad, inr

    def forward_kinematics(self, robot, conf):
        q = f64(conf).reshape(-1, robot.dof)
        M = q.shape[0]
        poses, J = np.zeros((M, robot.L, 4, 4)), np.zeros((M, robot.L, 6, robot.dof))
        self._ck(self.lib.gpmp2mi_forward_kinematics(robot.ptr, M, dptr(q), dptr(poses), dptr(J)))
        return poses, J

    def sphere_centers(self, robot, conf):
        q = f64(conf).reshape(-1, robot.dof)
        M = q.shape[0]
        c, J = np.zeros((M, robot.S, 3)), np.zeros((M, robot.S, 3, robot.dof))
        self._ck(self.lib.gpmp2mi_sphere_centers(robot.ptr, M, dptr(q), dptr(c), dptr(J)))
        return c, J

    def obstacle_factor(self, robot, sdf, epsilon, conf):
        q = f64(conf).reshape(-1, robot.dof)
        M = q.shape[0]
        err, H = np.zeros((M, robot.S)), np.zeros((M, robot.S, robot.dof))
        self._ck(self.lib.gpmp2mi_obstacle_factor(robot.ptr, sdf.ptr, C.c_double(epsilon), M, dptr(q),
                                                  dptr(err), dptr(H)))
        return err, H

    def obstacle_gp_factor(self, robot, sdf, epsilon, Qc, delta_t, tau, c1, v1, c2, v2):
        D = robot.dof
        c1, v1, c2, v2 = (f64(a).reshape(-1, D) for a in (c1, v1, c2, v2))
        M = c1.shape[0]
        Q = None if Qc is None else f64(Qc)
        err = np.zeros((M, robot.S))
        H = [np.zeros((M, robot.S, D)) for _ in range(4)]
        self._ck(self.lib.gpmp2mi_obstacle_gp_factor(robot.ptr, sdf.ptr, C.c_double(epsilon), dptr(Q),
                                                     C.c_double(delta_t), C.c_double(tau), M, dptr(c1),
                                                     dptr(v1), dptr(c2), dptr(v2), dptr(err),
                                                     *[dptr(h) for h in H]))
        return err, H

    def gp_prior_factor(self, dof, lie, delta_t, c1, v1, c2, v2):
        c1, v1, c2, v2 = (f64(a).reshape(-1, dof) for a in (c1, v1, c2, v2))
        M = c1.shape[0]
        err = np.zeros((M, 2 * dof))
        H = [np.zeros((M, 2 * dof, dof)) for _ in range(4)]
        self._ck(self.lib.gpmp2mi_gp_prior_factor(dof, int(lie), C.c_double(delta_t), M, dptr(c1), dptr(v1),
                                                  dptr(c2), dptr(v2), dptr(err), *[dptr(h) for h in H]))
        return err, H

    def gp_interpolate(self, dof, lie, Qc, delta_t, tau, c1, v1, c2, v2):
        c1, v1, c2, v2 = (f64(a).reshape(-1, dof) for a in (c1, v1, c2, v2))
        M = c1.shape[0]
        Q = None if Qc is None else f64(Qc)
        conf, vel = np.zeros((M, dof)), np.zeros((M, dof))
        self._ck(self.lib.gpmp2mi_gp_interpolate(dof, int(lie), dptr(Q), C.c_double(delta_t), C.c_double(tau),
                                                 M, dptr(c1), dptr(v1), dptr(c2), dptr(v2), dptr(conf), dptr(vel)))
        return conf, vel

    def interpolate_traj(self, dof, lie, Qc, delta_t, inter_step, traj, start_index=0, end_index=None):
        """traj [B][N+1][2D] -> [B][(end-start)*(inter_step+1)+1][2D]  (planner/TrajUtils.cpp:96-236)"""
        t = f64(traj)
        t = t.reshape(-1, t.shape[-2], 2 * dof)
        B, N = t.shape[0], t.shape[1] - 1
        end_index = N if end_index is None else int(end_index)
        Q = None if Qc is None else f64(Qc)
        out = np.zeros((B, max(end_index - start_index, 0) * (inter_step + 1) + 1, 2 * dof))
        self._ck(self.lib.gpmp2mi_interpolate_traj(dof, int(lie), dptr(Q), C.c_double(delta_t), int(inter_step), B, N,
                                               int(start_index), end_index, dptr(t), dptr(out)))
        return out

    def workspace_prior_factor(self, robot, mode, joint, des_pose, conf, jac=True):
        """mode 0 position / 1 orientation / 2 pose; des_pose 4x4 -> err [M][3|3|6], H [M][rows][D]"""
        q = f64(conf).reshape(-1, robot.dof)
        M, rows = q.shape[0], 6 if mode == 2 else 3
        des = f64(des_pose).reshape(4, 4)
        err, H = np.zeros((M, rows)), (np.zeros((M, rows, robot.dof)) if jac else None)
        self._ck(self.lib.gpmp2mi_workspace_prior_factor(robot.ptr, int(mode), int(joint), dptr(des), M, dptr(q), dptr(err),
                                                    dptr(H)))
        return err, H

    def goal_factor_arm(self, robot, dest_point, conf, jac=True):
        q = f64(conf).reshape(-1, robot.dof)
        M = q.shape[0]
        dest = f64(dest_point).reshape(3)
        err, H = np.zeros((M, 3)), (np.zeros((M, 3, robot.dof)) if jac else None)
        self._ck(self.lib.gpmp2mi_goal_factor_arm(robot.ptr, dptr(dest), M, dptr(q), dptr(err), dptr(H)))
        return err, H

    def self_collision_factor(self, robot, data, conf, jac=True):
        """data [n][4] = (sphere A, sphere B, epsilon, sigma) -> err [M][n], H [M][n][D]"""
        q = f64(conf).reshape(-1, robot.dof)
        d = f64(data).reshape(-1, 4)
        M, n = q.shape[0], d.shape[0]
        err, H = np.zeros((M, n)), (np.zeros((M, n, robot.dof)) if jac else None)
        self._ck(self.lib.gpmp2mi_self_collision_factor(robot.ptr, n, dptr(d), M, dptr(q), dptr(err), dptr(H)))
        return err, H

    def moving_sphere_factor(self, robot, radius, epsilon, conf, centers, jac=True):
        """The moving-sphere hinge (include/gpmp2mi.h "moving obstacles"): radius [K], conf [M][D], centers [M][K][3]
        (one centre set per evaluation) -> err [M][S][K], H [M][S][K][D]"""
        q = f64(conf).reshape(-1, robot.dof)
        M = q.shape[0]
        r = f64(radius).reshape(-1)
        K, S = r.size, int(robot.S)
        if K > scoring.MAX_MOVING_SPHERES:
            raise ValueError(f"{K} moving spheres, at most {scoring.MAX_MOVING_SPHERES}")
        c = f64(centers).reshape(M, K, 3)
        err, H = np.zeros((M, S, K)), (np.zeros((M, S, K, robot.dof)) if jac else None)
        self._ck(self.lib.gpmp2mi_moving_sphere_factor(robot.ptr, K, dptr(r), float(epsilon), M, dptr(q), dptr(c),
                                                       dptr(err), dptr(H)))
        return err, H

    def vehicle_dynamics_factor(self, lie, conf, vel):
        """sliding velocity of an SE(2) base -> err [M], Hp [M][D], Hv [M][D]"""
        q, v = f64(conf), f64(vel)
        q, v = q.reshape(-1, q.shape[-1]), v.reshape(-1, v.shape[-1])
        M, D = q.shape
        err, Hp, Hv = np.zeros(M), np.zeros((M, D)), np.zeros((M, D))
        self._ck(self.lib.gpmp2mi_vehicle_dynamics_factor(D, int(lie), M, dptr(q), dptr(v), dptr(err), dptr(Hp), dptr(Hv)))
        return err, Hp, Hv

    def joint_limit_factor(self, down, up, thresh, x):
        down, up, thresh = f64(down).reshape(-1), f64(up).reshape(-1), f64(thresh).reshape(-1)
        D = down.size
        x = f64(x).reshape(-1, D)
        err, Hd = np.zeros_like(x), np.zeros_like(x)
        self._ck(self.lib.gpmp2mi_joint_limit_factor(D, dptr(down), dptr(up), dptr(thresh), x.shape[0],
                                                     dptr(x), dptr(err), dptr(Hd)))
        return err, Hd

    def block_tridiag_solve(self, Hd, Ho, b):
        Hd, Ho, b = f64(Hd), f64(Ho), f64(b)
        B, nblk, n = Hd.shape[0], Hd.shape[1], Hd.shape[2]
        x, ok = np.zeros((B, nblk, n)), np.zeros(B, dtype=np.int32)
        self._ck(self.lib.gpmp2mi_block_tridiag_solve(B, nblk, n, dptr(Hd), dptr(Ho), dptr(b), dptr(x), iptr(ok)))
        return x, ok

    # ---------------------------------------------------------------- posterior (include/gpmp2mi.h "posterior")
    def block_tridiag_marginals(self, Hd, Ho, want=("Sdiag", "Soff", "ok")):
        """Sigma = H^-1 on the band of B block-tridiagonal SPD systems (layouts of block_tridiag_solve) ->
        dict(Sdiag [B][nblk][n][n], Soff [B][nblk-1][n][n] = block (i+1, i), ok [B]); want: the outputs to compute."""
        Hd, Ho = f64(Hd), f64(Ho)
        B, nblk, n = Hd.shape[0], Hd.shape[1], Hd.shape[2]
        o = dict(Sdiag=np.zeros((B, nblk, n, n)) if "Sdiag" in want else None,
                 Soff=np.zeros((B, nblk - 1, n, n)) if "Soff" in want else None,
                 ok=np.zeros(B, dtype=np.int32) if "ok" in want else None)
        self._ck(self.lib.gpmp2mi_block_tridiag_marginals(B, nblk, n, dptr(Hd), dptr(Ho), dptr(o["Sdiag"]),
                                                          dptr(o["Soff"]), iptr(o["ok"])))
        return o

    def block_tridiag_sample(self, Hd, Ho, z):
        """delta = L^-T z with H = L L^T, so cov(delta) = H^-1 for z ~ N(0, I): z [B][K][nblk][n] -> (delta, ok [B])"""
        Hd, Ho, z = f64(Hd), f64(Ho), f64(z)
        B, nblk, n = Hd.shape[0], Hd.shape[1], Hd.shape[2]
        if z.ndim != 4 or z.shape[0] != B or z.shape[2:] != (nblk, n):
            raise ValueError(f"z: expected [{B}][K][{nblk}][{n}], got {list(z.shape)}")
        delta, ok = np.zeros_like(z), np.zeros(B, dtype=np.int32)
        self._ck(self.lib.gpmp2mi_block_tridiag_sample(B, nblk, n, z.shape[1], dptr(Hd), dptr(Ho), dptr(z), dptr(delta),
                                                       iptr(ok)))
        return delta, ok

    # ------------------------------------------- the posterior on the executed timeline (include/gpmp2mi.h)
    def gp_interpolate_cov(self, dof, Qc, delta_t, inter_step, Sdiag, Soff):
        """The band of a posterior, Sdiag [B][N+1][2D][2D] and Soff [B][N][2D][2D] = block (i+1, i), carried to the
        Md = N (inter_step + 1) + 1 checked states: cov [B][Md][2D][2D], exactly symmetric, support states copied.
        Qc [D][D] or None (identity).  ValueError for mis-shaped arrays."""
        dof, inter_step = int(dof), _score_args(inter_step)
        if not float(delta_t) > 0:
            raise ValueError("delta_t must be > 0")
        B, N, Sd, So, q = band_inputs(dof, Sdiag, Soff, Qc)
        cov = np.zeros((B, scoring.checked_states(N, inter_step), 2 * dof, 2 * dof))
        self._ck(self.lib.gpmp2mi_gp_interpolate_cov(dof, dptr(q), float(delta_t), inter_step, B, N, dptr(Sd), dptr(So),
                                                     dptr(cov)))
        return cov

    def risk_traj(self, robot, sdf, Qc, delta_t, inter_step, traj, Sdiag, Soff, kappa, ok=None, want_sigma=True):
        """traj [B][N+1][2D] with the band of its posterior -> dict(robust_clearance [B] = min over the in-range pairs
        of clearance - kappa sigma, worst [B][2] = (checked state, sphere), sigma_worst [B], out_of_range [B],
        sigma [B][Md][S] or None); ok [B] or None: rows with ok == 0 answer NaN.  ValueError for mis-shaped arrays."""
        t = scoring.traj_rows(traj, robot.dof)
        inter_step, kappa = _score_args(inter_step), _kappa_arg(kappa)
        if not float(delta_t) > 0:
            raise ValueError("delta_t must be > 0")
        B, N, Sd, So, q = band_inputs(robot.dof, Sdiag, Soff, Qc)
        if t.shape[0] != B or t.shape[1] != N + 1:
            raise ValueError(f"traj: expected [{B}][{N + 1}][{2 * robot.dof}] to fit the band, got {list(t.shape)}")
        k = None
        if ok is not None:
            k = np.ascontiguousarray(ok, dtype=np.int32)
            if k.shape != (B,):
                raise ValueError(f"ok: expected [{B}], got {list(k.shape)}")
        Md = scoring.checked_states(N, inter_step)
        o = dict(robust_clearance=np.zeros(B), worst=np.zeros((B, 2), dtype=np.int32), sigma_worst=np.zeros(B),
                 out_of_range=np.zeros(B, dtype=np.int32), sigma=np.zeros((B, Md, robot.S)) if want_sigma else None)
        self._ck(self.lib.gpmp2mi_risk_traj(robot.ptr, sdf.ptr, dptr(q), float(delta_t), inter_step, B, N, dptr(t),
                                            dptr(Sd), dptr(So), iptr(k), kappa, dptr(o["robust_clearance"]),
                                            iptr(o["worst"]), dptr(o["sigma_worst"]), iptr(o["out_of_range"]),
                                            dptr(o["sigma"])))
        return o

    # ---------------------------------------------------------------- sampled clearance (include/gpmp2mi.h)
    def sampled_clearance_traj(self, robot, sdf, Qc, delta_t, inter_step, traj, delta, seed, required_clearance=0.0,
                               ok=None, row_first=0, sample_first=0, bridge=True, want_maps=True, want_conf=False):
        """traj [B][N+1][2D] with K support samples delta [B][K][N+1][2D] of its posterior -> dict(hits [B],
        probability [B], clearance [B][K], worst [B][K][2], state_clearance [B][K][Md] or None, state_hits [B][Md],
        oor_samples [B], conf [B][K][Md][D] or None): every sample carried to the Md checked states (bridge: with the
        noise of the prior bridge) and put through the collision check.  ok [B] or None: rows with ok == 0 answer -1 / NaN.
        ValueError for mis-shaped arrays."""
        t = scoring.traj_rows(traj, robot.dof)
        B, N, D = t.shape[0], t.shape[1] - 1, robot.dof
        de = f64(delta)
        if de.ndim != 4 or de.shape[0] != B or de.shape[1] < 1 or de.shape[2:] != (N + 1, 2 * D):
            raise ValueError(f"delta: expected [{B}][K][{N + 1}][{2 * D}] with K >= 1, got {list(de.shape)}")
        inter_step, K, row_first, sample_first, required_clearance = sampled_args(
            inter_step, de.shape[1], row_first, sample_first, required_clearance)
        if not float(delta_t) > 0:
            raise ValueError("delta_t must be > 0")
        q = None
        if Qc is not None:
            q = f64(Qc)
            if q.shape != (D, D):
                raise ValueError(f"Qc: expected [{D}][{D}], got {list(q.shape)}")
        k = None
        if ok is not None:
            k = np.ascontiguousarray(ok, dtype=np.int32)
            if k.shape != (B,):
                raise ValueError(f"ok: expected [{B}], got {list(k.shape)}")
        o = sampled_outputs(B, K, scoring.checked_states(N, inter_step), D, want_maps, want_conf)
        self._ck(self.lib.gpmp2mi_sampled_clearance_traj(
            robot.ptr, sdf.ptr, dptr(q), float(delta_t), inter_step, B, N, K, dptr(t), dptr(de), iptr(k), int(seed),
            row_first, sample_first, int(bool(bridge)), required_clearance, *_sampled_ptrs(o), dptr(o["conf"])))
        return o

    def sampled_chunk_bytes(self, nbytes=0):
        """Test hook: the byte budget of the delta chunk of Plan.collision_probability / sample_dense_seeded (0: default)."""
        self._ck(self.lib.gpmp2mi_debug_sampled_chunk_bytes(int(nbytes)))

    # ---------------------------------------------------------------- seeding (include/gpmp2mi.h "seeding")
    def normal_fill(self, seed, stream, a_first, a_count, b_first, b_count, nblk, n):
        """out [a_count][b_count][nblk][n] = normal(seed, stream, a_first + a, b_first + b, i, r): the library's counter
        RNG (gpmp2_amd/csrc/rng.h), evaluated on the device.  stream: _capi.RNG_RESTARTS / RNG_POSTERIOR or any id < 2^24."""
        out = np.zeros((int(a_count), int(b_count), int(nblk), int(n)))
        self._ck(self.lib.gpmp2mi_normal_fill(int(seed), int(stream), int(a_first), int(a_count), int(b_first),
                                              int(b_count), int(nblk), int(n), dptr(out)))
        return out

    def normal_fill_dev(self, seed, stream_id, a_first, a_count, b_first, b_count, nblk, n, out, stream=None):
        """The same into a device buffer (a torch tensor of that shape or a raw pointer); no host synchronisation."""
        shape = (int(a_count), int(b_count), int(nblk), int(n))
        if out is None:
            raise ValueError("out is required")
        self._ck(self.lib.gpmp2mi_normal_fill_dev(int(seed), int(stream_id), int(a_first), shape[0], int(b_first),
                                                  shape[1], shape[2], shape[3], _dev_arg("out", out, shape),
                                                  C.c_void_p(stream or 0)))

    def collision_cost(self, robot, sdf, total_step, traj):
        t = f64(traj).reshape(-1, total_step + 1, 2 * robot.dof)
        cost = np.zeros(t.shape[0])
        self._ck(self.lib.gpmp2mi_collision_cost(robot.ptr, sdf.ptr, total_step, t.shape[0], dptr(t), dptr(cost)))
        return cost

    # ---------------------------------------------------------------- scoring (include/gpmp2mi.h "scoring")
    def score_traj(self, robot, sdf, delta_t, inter_step, traj, out=None):
        """traj [B][N+1][2D] (or one [N+1][2D]) -> dict(support_cost [B], dense_cost [B], min_clearance [B],
        worst [B][2] = (checked state, sphere), out_of_range [B]) of the inter_step-up-sampled trajectories.
        out: a dict of caller arrays to fill instead (checked).  ValueError for mis-shaped arrays."""
        t = scoring.traj_rows(traj, robot.dof)
        inter_step = _score_args(inter_step)
        if not float(delta_t) > 0:
            raise ValueError("delta_t must be > 0")
        B, N = t.shape[0], t.shape[1] - 1
        o = scoring.score_outputs(B, out)
        self._ck(self.lib.gpmp2mi_score_traj(robot.ptr, sdf.ptr, float(delta_t), inter_step, B, N, dptr(t),
                                             *_score_ptrs(o)))
        return o

    def select_best(self, final_error, status, min_clearance, out_of_range=None, required_clearance=0.0,
                    require_in_range=False):
        """(best, n_eligible) by the selection rule (scoring.select_rule states it); host arrays, no device needed."""
        B, fe, st, clr, oor = scoring.select_inputs(final_error, status, min_clearance, out_of_range, require_in_range)
        best, n = C.c_int(-1), C.c_int(0)
        self._ck(self.lib.gpmp2mi_select_best(B, dptr(fe), iptr(st), dptr(clr), iptr(oor), float(required_clearance),
                                              int(bool(require_in_range)), C.byref(best), C.byref(n)))
        return best.value, n.value

    # ---------------------------------------------------------------- self-collision check (include/gpmp2mi.h)
    def _pairs_handle(self, out):
        h = _Handle(out, self.lib.gpmp2mi_self_pairs_destroy)
        h.P = int(self.lib.gpmp2mi_self_pairs_count(out))
        h.data = np.zeros((h.P, 4))
        self._ck(self.lib.gpmp2mi_self_pairs_get(out, dptr(h.data)))
        return h

    def self_pairs(self, robot, data):
        """A device-resident pair table for `robot` from data [P][4] = (sphere A, sphere B, epsilon, sigma): a handle
        with .P and .data.  An empty table is fine."""
        t = scoring.pair_table(data, getattr(robot, "S", None))
        out = C.c_void_p()
        self._ck(self.lib.gpmp2mi_self_pairs_create(robot.ptr, t.shape[0], dptr(t), C.byref(out)))
        return self._pairs_handle(out)

    def generate_self_pairs(self, robot, min_joint_gap=2, ref_conf=None, epsilon=0.0, sigma=1.0):
        """The table of all sphere pairs whose links are at least min_joint_gap joints apart in the robot's kinematic
        tree, less those that overlap at any of the reference configurations ref_conf [n][D] (None: none given)."""
        if int(min_joint_gap) < 1:
            raise ValueError("min_joint_gap must be >= 1")
        ref = np.zeros((0, robot.dof)) if ref_conf is None else f64(ref_conf).reshape(-1, robot.dof)
        out = C.c_void_p()
        self._ck(self.lib.gpmp2mi_self_pairs_generate(robot.ptr, int(min_joint_gap), ref.shape[0], dptr(ref),
                                                      float(epsilon), float(sigma), C.byref(out)))
        return self._pairs_handle(out)

    def self_score_traj(self, robot, pairs, delta_t, inter_step, traj, out=None):
        """traj [B][N+1][2D] (or one [N+1][2D]) -> dict(self_support_cost [B], self_dense_cost [B], min_self_clearance [B],
        worst [B][2] = (checked state, row of the table), invalid [B]) of the inter_step-up-sampled trajectories."""
        t = scoring.traj_rows(traj, robot.dof)
        inter_step = _score_args(inter_step)
        if not float(delta_t) > 0:
            raise ValueError("delta_t must be > 0")
        B, N = t.shape[0], t.shape[1] - 1
        o = scoring.score_outputs(B, out, scoring.SELF_NAMES)
        self._ck(self.lib.gpmp2mi_self_score_traj(robot.ptr, pairs.ptr, float(delta_t), inter_step, B, N, dptr(t),
                                                  *_self_ptrs(o)))
        return o

    # ---------------------------------------------------------------- motion limits (include/gpmp2mi.h)
    def motion_score_traj(self, robot, limits, delta_t, inter_step, traj, out=None):
        """traj [B][N+1][2D] (or one [N+1][2D]) -> dict(pos_margin [B], vel_ratio [B], acc_ratio [B], point_speed [B],
        time_scale [B], worst [B][4][2], invalid [B]) of the inter_step-up-sampled trajectories against `limits` (a
        MotionLimits; None: no limit)."""
        t = scoring.traj_rows(traj, robot.dof)
        inter_step = _score_args(inter_step)
        if not float(delta_t) > 0:
            raise ValueError("delta_t must be > 0")
        B, N = t.shape[0], t.shape[1] - 1
        o = scoring.motion_outputs(B, out)
        lim = _limits_arg(limits, robot.dof)
        self._ck(self.lib.gpmp2mi_motion_score_traj(robot.ptr, lim, float(delta_t), inter_step, B, N, dptr(t),
                                                    *_motion_ptrs(o)))
        return o

    # ---------------------------------------------------------------- torque limits (include/gpmp2mi.h)
    def dynamics(self, robot, mass, com, inertia, gravity=(0.0, 0.0, -9.81), torque=None):
        """A Dynamics handle for `robot`."""
        return Dynamics(self, robot, mass, com, inertia, gravity, torque)

    def torque_score_traj(self, robot, dynamics, delta_t, inter_step, traj, out=None, tau=True):
        """traj [B][N+1][2D] (or one [N+1][2D]) -> dict(torque_ratio [B], static_ratio [B], torque_time_scale [B], worst
        [B][3][2], invalid [B], tau [B][Md][D]) of the inter_step-up-sampled trajectories by inverse dynamics against the
        limits of `dynamics` (a Dynamics).  tau = False: the torques themselves are not fetched (tau: None)."""
        t = scoring.traj_rows(traj, robot.dof)
        inter_step = _score_args(inter_step)
        if not float(delta_t) > 0:
            raise ValueError("delta_t must be > 0")
        B, N = t.shape[0], t.shape[1] - 1
        o = scoring.torque_outputs(B, scoring.checked_states(N, inter_step), robot.dof, out, tau)
        self._ck(self.lib.gpmp2mi_torque_score_traj(robot.ptr, dynamics.ptr, float(delta_t), inter_step, B, N, dptr(t),
                                                    *_torque_ptrs(o)))
        return o

    # ---------------------------------------------------------------- re-timing (include/gpmp2mi.h)
    def retime_path(self, qd, qdd_left, qdd_right, cap, acc, h, max_rate=1.0, rate_start=None, rate_end=None, out=None):
        """The bare rule on any joint-space path: qd, qdd_left, qdd_right [B][Md][D] (or one [Md][D]), cap [B][Md] (a
        bound on sdot^2, inf: none), acc [D] or None -> dict(sdot, u, stamps [B][Md], duration [B], status [B],
        achieved [B][4])."""
        q = np.ascontiguousarray(qd, dtype=np.float64)
        q = q[None] if q.ndim == 2 else q
        if q.ndim != 3 or q.shape[1] < 2:
            raise ValueError(f"qd: expected [B][Md][D] with Md >= 2, got {list(np.shape(qd))}")
        B, Md, D = q.shape
        ql, qr = (np.ascontiguousarray(x, dtype=np.float64).reshape(q.shape) for x in (qdd_left, qdd_right))
        c = np.ascontiguousarray(cap, dtype=np.float64).reshape(B, Md)
        a = None if acc is None else scoring.motion_limits(D, acc=acc)[3]
        if not (np.isfinite(float(h)) and float(h) > 0):
            raise ValueError("h must be finite and > 0")
        rates = scoring.retime_rates(max_rate, rate_start, rate_end)
        o = scoring.retime_outputs(B, Md, None, out)
        self._ck(self.lib.gpmp2mi_retime_path(B, Md, D, dptr(q), dptr(ql), dptr(qr), dptr(c), dptr(a), float(h), *rates,
                                              *_retime_ptrs(o)))
        return o

    def retime_traj(self, robot, limits, delta_t, inter_step, traj, max_rate=1.0, rate_start=None, rate_end=None,
                    out=None):
        """traj [B][N+1][2D] (or one [N+1][2D]) -> dict(sdot, u, stamps [B][Md], duration [B], status [B], achieved
        [B][4], dense_retimed [B][Md][2D]): the fastest speed profile along the unchanged path under the rate limits of
        `limits` (a MotionLimits; None: max_rate alone).  rate_start / rate_end: a forced rate, None = free."""
        t = scoring.traj_rows(traj, robot.dof)
        inter_step = _score_args(inter_step)
        if not float(delta_t) > 0:
            raise ValueError("delta_t must be > 0")
        B, N = t.shape[0], t.shape[1] - 1
        rates = scoring.retime_rates(max_rate, rate_start, rate_end)
        o = scoring.retime_outputs(B, scoring.checked_states(N, inter_step), robot.dof, out)
        lim = _limits_arg(limits, robot.dof)
        self._ck(self.lib.gpmp2mi_retime_traj(robot.ptr, lim, float(delta_t), inter_step, B, N, dptr(t), *rates,
                                              *_retime_ptrs(o)))
        return o

    # ---------------------------------------------------------------- moving obstacles (include/gpmp2mi.h)
    def moving_score_traj(self, robot, radius, centers, epsilon, delta_t, inter_step, traj, out=None):
        """traj [B][N+1][2D] (or one [N+1][2D]) against the spheres radius [K], centers [K][N+1][3] -> dict(
        moving_support_cost [B], moving_dense_cost [B], min_moving_clearance [B], worst [B][3] = (checked state, robot
        sphere, moving sphere), invalid [B]) of the inter_step-up-sampled trajectories."""
        t = scoring.traj_rows(traj, robot.dof)
        inter_step = _score_args(inter_step)
        if not float(delta_t) > 0:
            raise ValueError("delta_t must be > 0")
        B, N = t.shape[0], t.shape[1] - 1
        K, r, c = scoring.moving_set(radius, centers, N + 1)
        o = scoring.score_outputs(B, out, scoring.MOVING_NAMES)
        self._ck(self.lib.gpmp2mi_moving_score_traj(robot.ptr, K, dptr(r), dptr(c), float(epsilon), float(delta_t),
                                                    inter_step, B, N, dptr(t), *_moving_ptrs(o)))
        return o

    # ---------------------------------------------------------------- workspace path (include/gpmp2mi.h)
    def workspace_path_factor(self, robot, mode, link, conf, des, jac=True):
        """The workspace-path factor with one target per evaluation (include/gpmp2mi.h "workspace path"): conf [M][D],
        des [M][4][4] -> err [M][rows], H [M][rows][D] (rows = 6 for mode 2, else 3)"""
        q = f64(conf).reshape(-1, robot.dof)
        M, rows = q.shape[0], 6 if int(mode) == 2 else 3
        d = f64(des).reshape(M, 16)
        err, H = np.zeros((M, rows)), (np.zeros((M, rows, robot.dof)) if jac else None)
        self._ck(self.lib.gpmp2mi_workspace_path_factor(robot.ptr, int(mode), int(link), M, dptr(q), dptr(d), dptr(err),
                                                        dptr(H)))
        return err, H

    def path_score_traj(self, robot, mode, link, des, sigma, delta_t, inter_step, traj, out=None):
        """traj [B][N+1][2D] (or one [N+1][2D]) against the path des [N+1][4][4], sigma [N+1] (or a scalar) -> dict(
        max_pos_dev [B], max_rot_dev [B], worst [B][2], support_cost [B], dense_cost [B], invalid [B]) of the
        inter_step-up-sampled trajectories."""
        t = scoring.traj_rows(traj, robot.dof)
        inter_step = _score_args(inter_step)
        if not float(delta_t) > 0:
            raise ValueError("delta_t must be > 0")
        B, N = t.shape[0], t.shape[1] - 1
        d, s = scoring.path_arrays(des, sigma, N + 1)
        o = scoring.path_outputs(B, out)
        self._ck(self.lib.gpmp2mi_path_score_traj(robot.ptr, int(mode), int(link), dptr(d), dptr(s), float(delta_t),
                                                  inter_step, B, N, dptr(t), *_path_ptrs(o)))
        return o

    # ---------------------------------------------------------------- distinct alternatives (include/gpmp2mi.h)
    def traj_distances(self, dof, traj, weights=None, metric=scoring.DIST_MAX_STATE):
        """traj [B][N+1][2 dof] -> dist [B][B] between the configuration halves (scoring.DIST_MAX_STATE / DIST_RMS)."""
        t = scoring.traj_rows(traj, dof)
        w, metric = scoring.group_weights(weights, dof), scoring.group_metric(metric)
        B, N = t.shape[0], t.shape[1] - 1
        dist = np.zeros((B, B))
        self._ck(self.lib.gpmp2mi_traj_distances(dof, B, N, dptr(t), dptr(w), metric, dptr(dist)))
        return dist

    def traj_distances_dev(self, dof, B, total_step, traj, dist, weights=None, metric=scoring.DIST_MAX_STATE, stream=None):
        """The same between device buffers (torch tensors or raw pointers); weights stays a host array."""
        w, metric = scoring.group_weights(weights, dof), scoring.group_metric(metric)
        B, N = int(B), int(total_step)
        args = [_dev_arg("traj", traj, (B, N + 1, 2 * dof)), dptr(w), metric, _dev_arg("dist", dist, (B, B))]
        self._ck(self.lib.gpmp2mi_traj_distances_dev(dof, B, N, *args, C.c_void_p(stream or 0)))

    def group_rows(self, dist, score, eligible=None, radius=0.0):
        """The leader rule (scoring.group_rule states it) on a given matrix; host arrays, no device needed:
        dict(mode [B], leaders [B], sizes [B], n_modes)."""
        B = int(np.shape(score)[0]) if np.ndim(score) == 1 else -1
        sc, el, d = scoring.group_inputs(B, score, eligible, dist, limit=False)
        radius = scoring.group_radius(radius)
        o, n = scoring.group_outputs(B), C.c_int(0)
        self._ck(self.lib.gpmp2mi_group_rows(B, dptr(d), dptr(sc), iptr(el), radius, iptr(o["mode"]), iptr(o["leaders"]),
                                             iptr(o["sizes"]), C.byref(n)))
        o["n_modes"] = n.value
        return o

    def group_rows_dev(self, B, dist, score, eligible=None, radius=0.0, mode=None, leaders=None, sizes=None, n_modes=None,
                       stream=None):
        """The same on device buffers, one kernel: dist [B][B], score [B], eligible int32 [B] or None; outputs int32
        mode / leaders / sizes [B], n_modes [1], any may be None."""
        B = int(B)
        if B > scoring.MAX_GROUP_ROWS:
            raise ValueError(f"at most {scoring.MAX_GROUP_ROWS} rows can be grouped, got {B}")
        args = [_dev_arg("dist", dist, (B, B)), _dev_arg("score", score, (B,)), _dev_arg("eligible", eligible, (B,), True),
                scoring.group_radius(radius), _dev_arg("mode", mode, (B,), True), _dev_arg("leaders", leaders, (B,), True),
                _dev_arg("sizes", sizes, (B,), True), _dev_arg("n_modes", n_modes, (1,), True)]
        self._ck(self.lib.gpmp2mi_group_rows_dev(B, *args, C.c_void_p(stream or 0)))

    def group_traj(self, dof, traj, score, eligible=None, radius=0.0, weights=None, metric=scoring.DIST_MAX_STATE):
        """Distances and rule on the device, without the [B][B] matrix: dict(mode, leaders, sizes, n_modes)."""
        t = scoring.traj_rows(traj, dof)
        w, metric = scoring.group_weights(weights, dof), scoring.group_metric(metric)
        B, N = t.shape[0], t.shape[1] - 1
        sc, el = scoring.group_inputs(B, score, eligible)
        radius = scoring.group_radius(radius)
        o, n = scoring.group_outputs(B), C.c_int(0)
        self._ck(self.lib.gpmp2mi_group_traj(dof, B, N, dptr(t), dptr(w), metric, radius, dptr(sc), iptr(el),
                                             iptr(o["mode"]), iptr(o["leaders"]), iptr(o["sizes"]), C.byref(n)))
        o["n_modes"] = n.value
        return o

    def group_traj_dev(self, dof, B, total_step, traj, score, eligible=None, radius=0.0, weights=None,
                       metric=scoring.DIST_MAX_STATE, mode=None, leaders=None, sizes=None, n_modes=None, stream=None):
        """The same on device buffers.  The bit matrix is allocated and freed inside the call: one synchronising
        allocation per call."""
        w, metric = scoring.group_weights(weights, dof), scoring.group_metric(metric)
        B, N = int(B), int(total_step)
        if B > scoring.MAX_GROUP_ROWS:
            raise ValueError(f"at most {scoring.MAX_GROUP_ROWS} rows can be grouped, got {B}")
        args = [_dev_arg("traj", traj, (B, N + 1, 2 * dof)), dptr(w), metric, scoring.group_radius(radius),
                _dev_arg("score", score, (B,)), _dev_arg("eligible", eligible, (B,), True),
                _dev_arg("mode", mode, (B,), True), _dev_arg("leaders", leaders, (B,), True),
                _dev_arg("sizes", sizes, (B,), True), _dev_arg("n_modes", n_modes, (1,), True)]
        self._ck(self.lib.gpmp2mi_group_traj_dev(dof, B, N, *args, C.c_void_p(stream or 0)))

    # ---------------------------------------------------------------- goal configurations (include/gpmp2mi.h)
    def ik_opts(self, robot, mode=_capi.WORKSPACE_POSE, link=None, limits=None, **kw):
        """gpmp2mi_ik_opts with the library's defaults: link defaults to the last one, limits = (down, up) or None, any
        other field by keyword (pos_tol, rot_tol, rot_weight, max_iter, lambda_initial / _factor / _lower / _upper).
        Returns (struct, keepalive)."""
        o = _capi.IkOptsC()
        self.lib.gpmp2mi_ik_opts_default(C.byref(o))
        o.mode, o.link = int(mode), int(robot.L - 1 if link is None else link)
        names = {n for n, _ in _capi.IkOptsC._fields_} - {"mode", "link", "pos_down", "pos_up"}
        for k, v in kw.items():
            if k not in names:
                raise ValueError(f"unknown IK option {k}")
            setattr(o, k, v)
        keep = None
        if limits is not None:
            keep = [f64(x).reshape(-1) for x in limits]
            if len(keep) != 2 or any(x.shape != (robot.dof,) for x in keep):
                raise ValueError(f"limits: expected (down [{robot.dof}], up [{robot.dof}])")
            o.pos_down, o.pos_up = dptr(keep[0]), dptr(keep[1])
        return o, keep

    @staticmethod
    def _ik_poses(des_pose):
        des = f64(des_pose)
        if des.shape == (4, 4):
            des = des.reshape(1, 4, 4)
        if des.ndim != 3 or des.shape[1:] != (4, 4):
            raise ValueError(f"des_pose: expected [G][4][4], got {list(des.shape)}")
        return des

    @staticmethod
    def _ik_seeds(seeds, G, D):
        s = f64(seeds)
        if s.ndim == 2 and G == 1:
            s = s.reshape(1, *s.shape)
        if s.ndim != 3 or s.shape[0] != G or s.shape[2] != D:
            raise ValueError(f"seeds: expected [{G}][M][{D}], got {list(s.shape)}")
        return s

    def ik_solve(self, robot, opts, des_pose, seeds=None, M=None, seed=0, first=0):
        """des_pose [G][4][4]; seeds [G][M][D], or None: M rows per pose drawn from (seed, first) inside the limits ->
        dict(conf [G][M][D], residual [G][M][2], iters [G][M], status [G][M])."""
        o, keep = opts if isinstance(opts, tuple) else (opts, None)
        des, D = self._ik_poses(des_pose), robot.dof
        G = des.shape[0]
        if seeds is not None:
            s = self._ik_seeds(seeds, G, D)
            M = s.shape[1]
        elif M is None or int(M) < 0 or int(first) < 0:
            raise ValueError("the seeded form needs M >= 0 and first >= 0")
        M = int(M)
        out = dict(conf=np.zeros((G, M, D)), residual=np.zeros((G, M, 2)), iters=np.zeros((G, M), dtype=np.int32),
                   status=np.zeros((G, M), dtype=np.int32))
        ptrs = (dptr(out["conf"]), dptr(out["residual"]), iptr(out["iters"]), iptr(out["status"]))
        if seeds is not None:
            self._ck(self.lib.gpmp2mi_ik_solve(robot.ptr, C.byref(o), G, dptr(des), M, dptr(s), *ptrs))
        else:
            self._ck(self.lib.gpmp2mi_ik_solve_seeded(robot.ptr, C.byref(o), G, dptr(des), M, int(seed), int(first), *ptrs))
        return out

    def ik_solve_dev(self, robot, opts, G, M, des_pose, seeds=None, seed=0, first=0, conf=None, residual=None, iters=None,
                     status=None, stream=None):
        """The same on device buffers (torch tensors or raw pointers), one enqueue: des_pose [G][16], seeds [G][M][D] or
        None (drawn); outputs conf [G][M][D], residual [G][M][2], int32 iters / status [G][M], any may be None."""
        o, keep = opts if isinstance(opts, tuple) else (opts, None)
        G, M, D = int(G), int(M), robot.dof
        outs = [_dev_arg("conf", conf, (G, M, D)), _dev_arg("residual", residual, (G, M, 2)),
                _dev_arg("iters", iters, (G, M), True), _dev_arg("status", status, (G, M), True)]
        des = _dev_arg("des_pose", des_pose, (G, 16))
        if seeds is not None:
            self._ck(self.lib.gpmp2mi_ik_solve_dev(robot.ptr, C.byref(o), G, des, M, _dev_arg("seeds", seeds, (G, M, D)),
                                                   *outs, C.c_void_p(stream or 0)))
        else:
            self._ck(self.lib.gpmp2mi_ik_solve_seeded_dev(robot.ptr, C.byref(o), G, des, M, int(seed), int(first), *outs,
                                                          C.c_void_p(stream or 0)))

    @staticmethod
    def _ik_goal_args(D, M, near, weights, radius, max_goals):
        if int(M) > scoring.MAX_GROUP_ROWS:
            raise ValueError(f"at most {scoring.MAX_GROUP_ROWS} seed rows per pose can be grouped, got {M}")
        if not 1 <= int(max_goals) <= scoring.MAX_ALTERNATIVES:
            raise ValueError(f"max_goals must be in 1..{scoring.MAX_ALTERNATIVES}")
        nr = None if near is None else f64(near).reshape(-1)
        if nr is not None and (nr.shape != (D,) or not np.isfinite(nr).all()):
            raise ValueError(f"near: expected {D} finite coordinates")
        return nr, scoring.group_weights(weights, D), scoring.group_radius(radius), int(max_goals)

    def ik_goals(self, robot, opts, des_pose, sdf=None, seeds=None, M=None, seed=0, first=0, radius=0.1, max_goals=8,
                 required_clearance=0.0, require_in_range=False, near=None, weights=None):
        """IK, the clearance of every answer, then one goal per distinct answer (the leader rule of scoring.group_rule per
        pose) -> dict(conf, status, clearance, out_of_range, mode [G][M]..; n_goals, n_converged, n_eligible [G];
        goal_conf [G][max_goals][D], goal_seed, goal_score, goal_clearance [G][max_goals]).  Slots beyond n_goals hold
        goal_seed = -1 and NaN."""
        o, keep = opts if isinstance(opts, tuple) else (opts, None)
        des, D = self._ik_poses(des_pose), robot.dof
        G = des.shape[0]
        s = None
        if seeds is not None:
            s = self._ik_seeds(seeds, G, D)
            M = s.shape[1]
        elif M is None or int(M) < 0 or int(first) < 0:
            raise ValueError("the seeded form needs M >= 0 and first >= 0")
        M = int(M)
        nr, w, radius, K = self._ik_goal_args(D, M, near, weights, radius, max_goals)
        i32 = lambda *shape: np.zeros(shape, dtype=np.int32)   # noqa: E731
        out = dict(conf=np.zeros((G, M, D)), status=i32(G, M), clearance=np.zeros((G, M)), out_of_range=i32(G, M),
                   mode=i32(G, M), n_goals=i32(G), n_converged=i32(G), n_eligible=i32(G),
                   goal_conf=np.full((G, K, D), np.nan), goal_seed=i32(G, K), goal_score=np.full((G, K), np.nan),
                   goal_clearance=np.full((G, K), np.nan))
        self._ck(self.lib.gpmp2mi_ik_goals(
            robot.ptr, C.byref(o), None if sdf is None else sdf.ptr, G, dptr(des), M, dptr(s), int(seed), int(first),
            float(required_clearance), int(bool(require_in_range)), dptr(nr), dptr(w), radius, K, dptr(out["conf"]),
            iptr(out["status"]), dptr(out["clearance"]), iptr(out["out_of_range"]), iptr(out["mode"]),
            iptr(out["n_goals"]), iptr(out["n_converged"]), iptr(out["n_eligible"]), dptr(out["goal_conf"]),
            iptr(out["goal_seed"]), dptr(out["goal_score"]), dptr(out["goal_clearance"])))
        return out

    def ik_goals_dev(self, robot, opts, G, M, des_pose, sdf=None, seeds=None, seed=0, first=0, radius=0.1, max_goals=8,
                     required_clearance=0.0, require_in_range=False, near=None, weights=None, conf=None, status=None,
                     clearance=None, out_of_range=None, mode=None, n_goals=None, n_converged=None, n_eligible=None,
                     goal_conf=None, goal_seed=None, goal_score=None, goal_clearance=None, stream=None):
        """The same on device buffers; near and weights stay host arrays.  The workspace is allocated and freed inside the
        call: one synchronising allocation per call."""
        o, keep = opts if isinstance(opts, tuple) else (opts, None)
        G, M, D = int(G), int(M), robot.dof
        nr, w, radius, K = self._ik_goal_args(D, M, near, weights, radius, max_goals)
        outs = [_dev_arg("conf", conf, (G, M, D)), _dev_arg("status", status, (G, M), True),
                _dev_arg("clearance", clearance, (G, M)), _dev_arg("out_of_range", out_of_range, (G, M), True),
                _dev_arg("mode", mode, (G, M), True), _dev_arg("n_goals", n_goals, (G,), True),
                _dev_arg("n_converged", n_converged, (G,), True), _dev_arg("n_eligible", n_eligible, (G,), True),
                _dev_arg("goal_conf", goal_conf, (G, K, D)), _dev_arg("goal_seed", goal_seed, (G, K), True),
                _dev_arg("goal_score", goal_score, (G, K)), _dev_arg("goal_clearance", goal_clearance, (G, K))]
        self._ck(self.lib.gpmp2mi_ik_goals_dev(
            robot.ptr, C.byref(o), None if sdf is None else sdf.ptr, G, _dev_arg("des_pose", des_pose, (G, 16)), M,
            _dev_arg("seeds", seeds, (G, M, D)), int(seed), int(first), float(required_clearance),
            int(bool(require_in_range)), dptr(nr), dptr(w), radius, K, *outs, C.c_void_p(stream or 0)))

    @staticmethod
    def goal_rows(goals, B, pose=0):
        """[B][D] end configurations for Plan.set_problem: the goals of pose `pose` (a dict of ik_goals) cycled over the B
        rows, row b taking goal b % min(n_goals, max_goals).  ValueError when the pose has no goal."""
        n = min(int(goals["n_goals"][pose]), goals["goal_conf"].shape[1])
        if n < 1:
            raise ValueError("no goal configuration was found for this pose")
        return np.ascontiguousarray(goals["goal_conf"][pose, np.arange(int(B)) % n])

    # ---------------------------------------------------------------- live map (include/gpmp2mi.h "live map")
    def _sdf_shape(self, sdf):
        """The voxel shape of a field handle, [nz][ny][nx] or [ny][nx]: kept by the calls that made it from an array, asked
        of the library once otherwise."""
        if getattr(sdf, "shape", None) is None:
            nx, ny, nz = C.c_int(), C.c_int(), C.c_int()
            self._ck(self.lib.gpmp2mi_sdf_get_field(sdf.ptr, None, C.byref(nx), C.byref(ny), C.byref(nz), None, None, None))
            sdf.shape = (nz.value, ny.value, nx.value)[3 - sdf.dim:]
        return tuple(sdf.shape)

    def _grid_arg(self, sdf, name, a, layout):
        a, shape = f64(a), self._sdf_shape(sdf)
        if layout not in (_capi.SDF_LAYOUT_ZYX, _capi.SDF_LAYOUT_GTSAM):
            raise ValueError("unknown voxel layout")
        if a.ndim != len(shape) or a.size != int(np.prod(shape)) or (layout == _capi.SDF_LAYOUT_ZYX and a.shape != shape):
            raise ValueError(f"{name}: expected {list(shape)} (the handle's grid), got {list(a.shape)}")
        return a

    def _points_args(self, sdf, robot, conf, margin):
        margin = float(margin)
        if np.isnan(margin):
            raise ValueError("margin must not be NaN")
        if robot is not None and conf is None:
            raise ValueError("the self filter needs the robot's configuration")
        return margin

    def sdf_reserve_update(self, sdf):
        """Takes the update workspace of the handle now, so that the first `_dev` update does not allocate."""
        self._ck(self.lib.gpmp2mi_sdf_reserve_update(sdf.ptr))

    def sdf_update(self, sdf, data, layout=_capi.SDF_LAYOUT_ZYX):
        """New voxels of the handle's own shape, in place; the handle then equals Engine.sdf of the same data."""
        data = self._grid_arg(sdf, "data", data, layout)
        self._ck(self.lib.gpmp2mi_sdf_update(sdf.ptr, dptr(data), C.c_int(layout)))

    def sdf_update_dev(self, sdf, data, stream=None):
        """The same from a device buffer in [nz][ny][nx] order (torch tensor or raw pointer), enqueued on `stream`."""
        self._ck(self.lib.gpmp2mi_sdf_update_dev(sdf.ptr, _dev_arg("data", data, self._sdf_shape(sdf)),
                                                 C.c_void_p(stream or 0)))

    def sdf_update_from_occupancy(self, sdf, occ, layout=_capi.SDF_LAYOUT_ZYX):
        """The handle's field from an occupancy grid of its own shape, in place (as Engine.sdf_from_occupancy); the
        obstacle set becomes the handle's base."""
        occ = self._grid_arg(sdf, "occ", occ, layout)
        self._ck(self.lib.gpmp2mi_sdf_update_from_occupancy(sdf.ptr, dptr(occ), C.c_int(layout)))

    def sdf_update_from_occupancy_dev(self, sdf, occ, stream=None):
        self._ck(self.lib.gpmp2mi_sdf_update_from_occupancy_dev(sdf.ptr, _dev_arg("occ", occ, self._sdf_shape(sdf)),
                                                                C.c_void_p(stream or 0)))

    def sdf_update_from_points(self, sdf, points, use_base=True, robot=None, conf=None, margin=0.0):
        """The handle's field from a point cloud [M][dim] (and the base when use_base), in place.  robot / conf: drop the
        points inside the robot's body spheres grown by `margin`.  -> dict(kept, non_finite, self, outside)."""
        margin = self._points_args(sdf, robot, conf, margin)
        p = f64(points)
        if p.size == 0:
            p = p.reshape(0, sdf.dim)
        if p.ndim != 2 or p.shape[1] != sdf.dim:
            raise ValueError(f"points: expected [M][{sdf.dim}], got {list(p.shape)}")
        q = None
        if robot is not None:
            q = f64(conf).reshape(-1)
            if q.size != robot.dof:
                raise ValueError(f"conf: expected [{robot.dof}], got {list(np.shape(conf))}")
        stats = np.zeros(4, dtype=np.int32)
        self._ck(self.lib.gpmp2mi_sdf_update_from_points(sdf.ptr, p.shape[0], dptr(p), int(bool(use_base)),
                                                         None if robot is None else robot.ptr, dptr(q), margin,
                                                         iptr(stats)))
        return dict(zip(("kept", "non_finite", "self", "outside"), (int(x) for x in stats)))

    def sdf_update_from_points_dev(self, sdf, M, points, use_base=True, robot=None, conf=None, margin=0.0, stats=None,
                                   stream=None):
        """The same from device buffers (torch tensors or raw pointers): points [M][dim], conf [dof], stats [4] int32 or
        None; enqueued on `stream`, no host synchronisation."""
        margin, M = self._points_args(sdf, robot, conf, margin), int(M)
        if M < 0:
            raise ValueError("M must be >= 0")
        args = [_dev_arg("points", points, (M, sdf.dim)), int(bool(use_base)), None if robot is None else robot.ptr,
                None if robot is None else _dev_arg("conf", conf, (robot.dof,)), margin,
                _dev_arg("stats", stats, (4,), True)]
        self._ck(self.lib.gpmp2mi_sdf_update_from_points_dev(sdf.ptr, M, *args, C.c_void_p(stream or 0)))

    def sdf_update_timing(self, sdf, on=True, read=False):
        """Stage timer of the updates (gpmp2mi_debug_sdf_update_timing): read = True returns the device times in ms of the
        last recorded update as dict(seed_mark, passes, finish, pack)."""
        ms = np.zeros(4) if read else None
        self._ck(self.lib.gpmp2mi_debug_sdf_update_timing(sdf.ptr, int(bool(on)), dptr(ms)))
        return None if ms is None else dict(zip(("seed_mark", "passes", "finish", "pack"), (float(x) for x in ms)))

    # ---------------------------------------------------------------- sensor map (include/gpmp2mi.h "sensor map")
    EVIDENCE_DEFAULTS = dict(hit=2, miss=1, lo=-4, hi=8, occupied_at=1, use_base=False, refresh=True)
    EVIDENCE_STATS = ("hit", "invalid", "max_range", "self", "outside", "occupied")

    @classmethod
    def _evidence_opts(cls, opts):
        unknown = set(opts) - set(cls.EVIDENCE_DEFAULTS)
        if unknown:
            raise ValueError(f"unknown evidence options: {sorted(unknown)}")
        o = _capi.EvidenceOpts()
        for k, v in dict(cls.EVIDENCE_DEFAULTS, **opts).items():
            setattr(o, k, int(v))
        return o

    @staticmethod
    def _camera(camera):
        """dict(width, height, fx, fy, cx, cy, depth_min, depth_max, pose [3][4] camera -> world) -> DepthCamera"""
        pose = f64(camera["pose"])
        if pose.size != 12:
            raise ValueError(f"camera pose: expected [3][4], got {list(pose.shape)}")
        cam = _capi.DepthCamera()
        cam.width, cam.height = int(camera["width"]), int(camera["height"])
        for k in ("fx", "fy", "cx", "cy", "depth_min", "depth_max"):
            setattr(cam, k, float(camera[k]))
        for k, v in enumerate(pose.reshape(12)):
            cam.pose[k] = float(v)
        return cam

    def _sensor_origin(self, sdf, sensor_origin):
        o = f64(sensor_origin).reshape(-1)
        if o.size != sdf.dim:
            raise ValueError(f"sensor_origin: expected [{sdf.dim}], got {list(np.shape(sensor_origin))}")
        return o

    def _conf_arg(self, robot, conf):
        if robot is None:
            return None
        q = f64(conf).reshape(-1)
        if q.size != robot.dof:
            raise ValueError(f"conf: expected [{robot.dof}], got {list(np.shape(conf))}")
        return q

    def sdf_reserve_evidence(self, sdf):
        """Takes the evidence workspace of the handle now, so that the first `_dev` integrate call does not allocate."""
        self._ck(self.lib.gpmp2mi_sdf_reserve_evidence(sdf.ptr))

    def sdf_integrate_points(self, sdf, points, sensor_origin, robot=None, conf=None, margin=0.0, **opts):
        """One frame of rays from sensor_origin [dim] to points [M][dim] into the handle's evidence: +hit where a ray
        ends, -miss where rays pass, clamped; then (refresh) the field again from the cells with evidence >= occupied_at.
        opts: hit, miss, lo, hi, occupied_at, use_base, refresh (EVIDENCE_DEFAULTS).  robot / conf / margin: rays that
        end inside the robot's body spheres carve and do not mark.
        -> dict(hit, invalid, max_range, self, outside, occupied)."""
        margin = self._points_args(sdf, robot, conf, margin)
        p = f64(points)
        if p.size == 0:
            p = p.reshape(0, sdf.dim)
        if p.ndim != 2 or p.shape[1] != sdf.dim:
            raise ValueError(f"points: expected [M][{sdf.dim}], got {list(p.shape)}")
        o, q, eo = self._sensor_origin(sdf, sensor_origin), self._conf_arg(robot, conf), self._evidence_opts(opts)
        stats = np.zeros(6, dtype=np.int32)
        self._ck(self.lib.gpmp2mi_sdf_integrate_points(sdf.ptr, p.shape[0], dptr(p), dptr(o),
                                                       None if robot is None else robot.ptr, dptr(q), margin,
                                                       C.byref(eo), iptr(stats)))
        return dict(zip(self.EVIDENCE_STATS, (int(x) for x in stats)))

    def sdf_integrate_points_dev(self, sdf, M, points, sensor_origin, robot=None, conf=None, margin=0.0, stats=None,
                                 stream=None, **opts):
        """The same from device buffers (torch tensors or raw pointers): points [M][dim], conf [dof], stats [6] int32 or
        None; sensor_origin is a host array.  Enqueued on `stream`, no host synchronisation."""
        margin, M = self._points_args(sdf, robot, conf, margin), int(M)
        if M < 0:
            raise ValueError("M must be >= 0")
        o, eo = self._sensor_origin(sdf, sensor_origin), self._evidence_opts(opts)
        self._ck(self.lib.gpmp2mi_sdf_integrate_points_dev(
            sdf.ptr, M, _dev_arg("points", points, (M, sdf.dim)), dptr(o), None if robot is None else robot.ptr,
            None if robot is None else _dev_arg("conf", conf, (robot.dof,)), margin, C.byref(eo),
            _dev_arg("stats", stats, (6,), True), C.c_void_p(stream or 0)))

    def sdf_integrate_depth(self, sdf, camera, depth, robot=None, conf=None, margin=0.0, **opts):
        """One depth image [height][width] (float32 metres along the optical axis) of `camera` (a dict: width, height,
        fx, fy, cx, cy, depth_min, depth_max, pose [3][4] camera -> world) into the evidence of a 3-D handle, as
        sdf_integrate_points; pixels beyond depth_max carve up to depth_max and mark no end."""
        margin = self._points_args(sdf, robot, conf, margin)
        cam = self._camera(camera)
        z = np.ascontiguousarray(depth, dtype=np.float32)
        if sdf.dim != 3:
            raise ValueError("the depth form needs a 3-D field")
        if z.shape != (cam.height, cam.width):
            raise ValueError(f"depth: expected [{cam.height}][{cam.width}], got {list(z.shape)}")
        q, eo = self._conf_arg(robot, conf), self._evidence_opts(opts)
        stats = np.zeros(6, dtype=np.int32)
        self._ck(self.lib.gpmp2mi_sdf_integrate_depth(sdf.ptr, C.byref(cam), z.ctypes.data_as(C.POINTER(C.c_float)),
                                                      None if robot is None else robot.ptr, dptr(q), margin,
                                                      C.byref(eo), iptr(stats)))
        return dict(zip(self.EVIDENCE_STATS, (int(x) for x in stats)))

    def sdf_integrate_depth_dev(self, sdf, camera, depth, robot=None, conf=None, margin=0.0, stats=None, stream=None,
                                **opts):
        """The same from device buffers: depth a contiguous float32 cuda tensor [height][width] or a raw pointer."""
        margin = self._points_args(sdf, robot, conf, margin)
        cam, eo = self._camera(camera), self._evidence_opts(opts)
        if hasattr(depth, "data_ptr"):
            if (str(depth.dtype) != "torch.float32" or not depth.is_contiguous() or depth.device.type != "cuda"
                    or tuple(depth.shape) != (cam.height, cam.width)):
                raise ValueError(f"depth: expected a contiguous torch.float32 cuda tensor of shape "
                                 f"{[cam.height, cam.width]}, got {depth.dtype} {list(depth.shape)} on {depth.device}")
            depth = depth.data_ptr()
        self._ck(self.lib.gpmp2mi_sdf_integrate_depth_dev(
            sdf.ptr, C.byref(cam), C.c_void_p(int(depth)), None if robot is None else robot.ptr,
            None if robot is None else _dev_arg("conf", conf, (robot.dof,)), margin, C.byref(eo),
            _dev_arg("stats", stats, (6,), True), C.c_void_p(stream or 0)))

    def sdf_refresh_from_evidence(self, sdf, occupied_at=1, use_base=False, stream=None, dev=False):
        """The field again from the evidence as it stands: the cells with evidence >= occupied_at, united with the base
        when use_base.  dev = True: enqueued on `stream` without a host synchronisation."""
        if dev:
            self._ck(self.lib.gpmp2mi_sdf_refresh_from_evidence_dev(sdf.ptr, int(occupied_at), int(bool(use_base)),
                                                                    C.c_void_p(stream or 0)))
        else:
            self._ck(self.lib.gpmp2mi_sdf_refresh_from_evidence(sdf.ptr, int(occupied_at), int(bool(use_base))))

    def sdf_evidence_reset(self, sdf, stream=None, dev=False):
        """Evidence 0 everywhere; the field stays as it is."""
        if dev:
            self._ck(self.lib.gpmp2mi_sdf_evidence_reset_dev(sdf.ptr, C.c_void_p(stream or 0)))
        else:
            self._ck(self.lib.gpmp2mi_sdf_evidence_reset(sdf.ptr))

    def sdf_evidence(self, sdf):
        """-> the handle's evidence, int16 [nz][ny][nx] or [ny][nx] (all 0 before the first integrate call)"""
        E = np.zeros(self._sdf_shape(sdf), dtype=np.int16)
        self._ck(self.lib.gpmp2mi_sdf_get_evidence(sdf.ptr, E.ctypes.data_as(C.POINTER(C.c_int16))))
        return E

    def sdf_integrate_timing(self, sdf, on=True, read=False):
        """Stage timer of the integrate calls (gpmp2mi_debug_sdf_integrate_timing): read = True returns the device times
        in ms of the last recorded call with refresh as dict(deproject, walk, apply_seed, passes, finish, pack)."""
        ms = np.zeros(6) if read else None
        self._ck(self.lib.gpmp2mi_debug_sdf_integrate_timing(sdf.ptr, int(bool(on)), dptr(ms)))
        names = ("deproject", "walk", "apply_seed", "passes", "finish", "pack")
        return None if ms is None else dict(zip(names, (float(x) for x in ms)))

    # ---------------------------------------------------------------- scene (include/gpmp2mi.h "scene")
    def scene(self, objects):
        """A scene handle of Box / Sphere / Cylinder / Mesh objects (gpmp2_amd.scene) on the current device."""
        from . import scene as _scene
        return _scene.Scene(objects, self)

    def sdf_update_from_scene(self, sdf, scene, use_base=False, use_evidence=False, occupied_at=1):
        """The handle's field from the scene's enabled objects, united with the base (use_base) and with the cells whose
        evidence is >= occupied_at (use_evidence), in place.  -> cells [K] int32: the count of each object alone
        (0 disabled, -1 a mesh out of range)."""
        cells = np.zeros(scene.K, dtype=np.int32)
        self._ck(self.lib.gpmp2mi_sdf_update_from_scene(sdf.ptr, scene.ptr, int(bool(use_base)), int(bool(use_evidence)),
                                                        int(occupied_at), iptr(cells)))
        return cells

    def sdf_update_from_scene_dev(self, sdf, scene, use_base=False, use_evidence=False, occupied_at=1, cells=None,
                                  stream=None):
        """The same enqueued on `stream` without a host synchronisation; cells: a device buffer [K] int32 or None."""
        self._ck(self.lib.gpmp2mi_sdf_update_from_scene_dev(sdf.ptr, scene.ptr, int(bool(use_base)),
                                                            int(bool(use_evidence)), int(occupied_at),
                                                            _dev_arg("cells", cells, (scene.K,), True),
                                                            C.c_void_p(stream or 0)))

    def scene_rasterize_dev(self, scene, origin, cell_size, shape, mask, cells=None, stream=None):
        """The scene alone into a device byte mask of `shape` ([nz][ny][nx] or [ny][nx]; a contiguous torch.uint8 cuda
        tensor or a raw pointer) on `stream`; cells: a device buffer [K] int32 or None."""
        shape = tuple(int(x) for x in shape)
        dim = len(shape)
        origin = f64(origin).reshape(-1)
        if dim not in (2, 3) or origin.size != dim:
            raise ValueError(f"a shape of 2 or 3 sizes and an origin of as many numbers, got {shape}, {origin.size}")
        if hasattr(mask, "data_ptr"):
            if (str(mask.dtype) != "torch.uint8" or not mask.is_contiguous() or mask.device.type != "cuda"
                    or tuple(mask.shape) != shape):
                raise ValueError(f"mask: expected a contiguous torch.uint8 cuda tensor of shape {list(shape)}, got "
                                 f"{mask.dtype} {list(mask.shape)} on {mask.device}")
            mask = mask.data_ptr()
        nz, ny, nx = ((1,) + shape) if dim == 2 else shape
        org = f64(list(origin) + [0.0] * (3 - dim))
        self._ck(self.lib.gpmp2mi_scene_rasterize_dev(scene.ptr, dim, dptr(org), float(cell_size), nx, ny, nz,
                                                      C.c_void_p(int(mask)), _dev_arg("cells", cells, (scene.K,), True),
                                                      C.c_void_p(stream or 0)))

    def scene_timing(self, scene, on=True, read=False):
        """Stage timer of the rasterisation (gpmp2mi_debug_scene_timing): read = True returns the device times in ms of
        the last recorded call as dict(primitives, meshes)."""
        ms = np.zeros(2) if read else None
        self._ck(self.lib.gpmp2mi_debug_scene_timing(scene.ptr, int(bool(on)), dptr(ms)))
        return None if ms is None else dict(zip(("primitives", "meshes"), (float(x) for x in ms)))

    # ---------------------------------------------------------------- plans
    def plan(self, robot, sdf, setting, B, forms=None):
        return Plan(self, robot, sdf, setting, B, forms)

    def multi_plan(self, robot, sdf, setting, B, devices, forms=None, replicate_all=False):
        """B trajectories sharded over `devices` (one plan per entry, repeats allowed): MultiPlan."""
        return MultiPlan(self, robot, sdf, setting, B, devices, forms, replicate_all)

    def replica_counts(self):
        """(robot, field) copies owned by live multi plans (gpmp2mi_debug_replica_counts)."""
        r, s = C.c_long(), C.c_long()
        self._ck(self.lib.gpmp2mi_debug_replica_counts(C.byref(r), C.byref(s)))
        return r.value, s.value

    # graph-level helpers with the oracle's call shape; forms: see Plan
    def _plan_for(self, robot, sdf, setting, start_conf, start_vel, end_conf, end_vel, traj, forms=None):
        D = setting.dof
        sc = f64(start_conf).reshape(-1, D)
        pl = Plan(self, robot, sdf, setting, sc.shape[0], forms)
        t = f64(traj).reshape(sc.shape[0], setting.total_step + 1, 2 * D)
        pl.set_problem(start_conf, start_vel, end_conf, end_vel, t)
        return pl, t

    def graph_error(self, robot, sdf, setting, start_conf, start_vel, end_conf, end_vel, traj, forms=None):
        pl, t = self._plan_for(robot, sdf, setting, start_conf, start_vel, end_conf, end_vel, traj, forms)
        return pl.graph_error(t)

    def linearize(self, robot, sdf, setting, start_conf, start_vel, end_conf, end_vel, traj, forms=None):
        pl, t = self._plan_for(robot, sdf, setting, start_conf, start_vel, end_conf, end_vel, traj, forms)
        return pl.linearize(t)

    def batch_optimize(self, robot, sdf, setting, start_conf, start_vel, end_conf, end_vel, init, forms=None):
        pl, t = self._plan_for(robot, sdf, setting, start_conf, start_vel, end_conf, end_vel, init, forms)
        pl.optimize()
        return pl.result()

    def queue_optimize(self, robot, sdf, setting, slots, start_conf, start_vel, end_conf, end_vel, init, forms=None):
        """M problems ([M][D] x 4, [M][N+1][2D]) through one plan of `slots` trajectories (Plan.optimize_queue): the
        result() dict with M rows, plus the run's queue_stats() under "stats"."""
        queue_inputs(setting.dof, setting.total_step, start_conf, start_vel, end_conf, end_vel, init)
        pl = Plan(self, robot, sdf, setting, slots, forms)
        try:
            res = pl.optimize_queue(start_conf, start_vel, end_conf, end_vel, init)
            res["stats"] = pl.queue_stats()
        finally:
            pl.close()
        return res


class Plan:
    """gpmp2mi_plan: B trajectory problems resident on the GPU.  forms (tests, probes): a dict of the kernel forms to force
    on the plan, e.g. {"lin_split": 2} (gpmp2mi_debug_forms, include/gpmp2mi_debug.h); None: the plan's own choice."""

    def __init__(self, eng: Engine, robot, sdf, setting, B: int, forms=None):
        self.eng, self.robot, self.sdf, self.setting, self.B = eng, robot, sdf, setting, int(B)
        s, o, keep = _capi.make_settings(setting)
        self._keep = (s, o, keep)
        out = C.c_void_p()
        if forms is None:
            eng._ck(eng.lib.gpmp2mi_plan_create(robot.ptr, sdf.ptr, C.byref(s), C.byref(o), self.B, C.byref(out)))
        else:
            f = _capi.make_debug_forms(forms)
            eng._ck(eng.lib.gpmp2mi_debug_plan_create(robot.ptr, sdf.ptr, C.byref(s), C.byref(o), self.B, C.byref(f),
                                                      C.byref(out)))
        self.h = _Handle(out, eng.lib.gpmp2mi_plan_destroy)
        self.D, self.N = setting.dof, setting.total_step

    def close(self):
        self.h.close()

    def set_problem(self, start_conf, start_vel, end_conf, end_vel, init):
        D, B = self.D, self.B
        a = [f64(x).reshape(B, D) for x in (start_conf, start_vel, end_conf, end_vel)]
        t = f64(init).reshape(B, self.N + 1, 2 * D)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_set_problem(self.h.ptr, *[dptr(x) for x in a], dptr(t)))

    def set_problem_dev(self, start_conf, start_vel, end_conf, end_vel, init, stream=None):
        """device pointers (ints, e.g. torch.Tensor.data_ptr()) of contiguous fp64 buffers."""
        args = [C.c_void_p(int(x)) for x in (start_conf, start_vel, end_conf, end_vel, init)]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_set_problem_dev(self.h.ptr, *args, C.c_void_p(stream or 0)))

    def optimize(self, stream=None):
        self.eng._ck(self.eng.lib.gpmp2mi_plan_optimize(self.h.ptr, C.c_void_p(stream or 0)))

    def result(self):
        B, D, N = self.B, self.D, self.N
        traj = np.zeros((B, N + 1, 2 * D))
        iters, status = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        ferr, trace = np.zeros(B), np.zeros((B, self.setting.max_iter + 1))
        self.eng._ck(self.eng.lib.gpmp2mi_plan_get_result(self.h.ptr, dptr(traj), iptr(iters), dptr(ferr),
                                                          iptr(status), dptr(trace)))
        return dict(traj=traj, iters=iters, final_error=ferr, status=status, error_trace=trace)

    def result_counts(self):
        B = self.B
        iters, status, ferr = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), np.zeros(B)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_get_result(self.h.ptr, None, iptr(iters), dptr(ferr), iptr(status), None))
        return iters, status, ferr

    # ---- a queue of problems through the plan's B slots (gpmp2mi_plan_optimize_queue, include/gpmp2mi.h)
    def optimize_queue(self, start_conf, start_vel, end_conf, end_vel, init):
        """M problems ([M][D] x 4, [M][N+1][2D], host arrays): the result() dict with M rows, row j = problem j."""
        M, (sc, sv, ec, ev), t = queue_inputs(self.D, self.N, start_conf, start_vel, end_conf, end_vel, init)
        D, N = self.D, self.N
        traj = np.zeros((M, N + 1, 2 * D))
        iters, status = np.zeros(M, dtype=np.int32), np.zeros(M, dtype=np.int32)
        ferr, trace = np.zeros(M), np.zeros((M, self.setting.max_iter + 1))
        self.eng._ck(self.eng.lib.gpmp2mi_plan_optimize_queue(self.h.ptr, M, dptr(sc), dptr(sv), dptr(ec), dptr(ev),
                                                              dptr(t), dptr(traj), iptr(iters), dptr(ferr), iptr(status),
                                                              dptr(trace)))
        return dict(traj=traj, iters=iters, final_error=ferr, status=status, error_trace=trace)

    def optimize_queue_dev(self, M, start_conf, start_vel, end_conf, end_vel, init, traj=None, iters=None,
                           final_error=None, status=None, error_trace=None, stream=None):
        """The same on device buffers: torch tensors (checked for device, dtype, contiguity and shape) or raw device
        pointers (ints); outputs may be None.  stream: a hipStream_t as int (e.g. torch.cuda.Stream.cuda_stream)."""
        D, N, T = self.D, self.N, self.setting.max_iter + 1
        M = int(M)
        if M < 1:
            raise ValueError("M must be >= 1")
        shapes = [(M, D)] * 4 + [(M, N + 1, 2 * D), (M, N + 1, 2 * D), (M,), (M,), (M,), (M, T)]
        names = ["start_conf", "start_vel", "end_conf", "end_vel", "init", "traj", "iters", "final_error", "status",
                 "error_trace"]
        ints = {"iters", "status"}
        args = []
        for name, shape, x in zip(names, shapes, (start_conf, start_vel, end_conf, end_vel, init, traj, iters,
                                                  final_error, status, error_trace)):
            if x is None:
                if len(args) < 5:
                    raise ValueError(f"{name} is required")
                args.append(None)
                continue
            if hasattr(x, "data_ptr"):
                want = "torch.int32" if name in ints else "torch.float64"
                if str(x.dtype) != want or not x.is_contiguous() or tuple(x.shape) != shape or x.device.type != "cuda":
                    raise ValueError(f"{name}: expected a contiguous {want} cuda tensor of shape {list(shape)}, got "
                                     f"{x.dtype} {list(x.shape)} on {x.device}")
                x = x.data_ptr()
            args.append(C.c_void_p(int(x)))
        self.eng._ck(self.eng.lib.gpmp2mi_plan_optimize_queue_dev(self.h.ptr, M, *args, C.c_void_p(stream or 0)))

    # ---- restarts drawn on the device from the GP prior (include/gpmp2mi.h "seeding")
    def seed_restarts(self, M, seed, start_conf=None, end_conf=None, mean=None, first=0, scale=1.0, keep_first=False):
        """init [M][N+1][2D]: problem j = first + row gets mean_j + scale * L^-T z_j, z_j from the counter RNG at
        (seed, j); mean None: the straight line from start_conf[row] to end_conf[row] ([M][D])."""
        M, sc, ec, mu = seed_inputs(self.D, self.N, start_conf, end_conf, mean, M)
        init = np.zeros((M, self.N + 1, 2 * self.D))
        self.eng._ck(self.eng.lib.gpmp2mi_plan_seed_restarts(self.h.ptr, M, int(seed), int(first), float(scale),
                                                             int(bool(keep_first)), dptr(sc), dptr(ec), dptr(mu),
                                                             dptr(init)))
        return init

    def seed_restarts_dev(self, M, seed, init, start_conf=None, end_conf=None, mean=None, first=0, scale=1.0,
                          keep_first=False, stream=None):
        """The same on device buffers (torch tensors or raw pointers); no host synchronisation after the plan's first
        seeded call."""
        D, N, M = self.D, self.N, int(M)
        if M < 1:
            raise ValueError("M must be >= 1")
        if init is None or (mean is None and (start_conf is None or end_conf is None)):
            raise ValueError("init, and start_conf / end_conf unless a mean is given, are required")
        args = [_dev_arg("start_conf", start_conf, (M, D)), _dev_arg("end_conf", end_conf, (M, D)),
                _dev_arg("mean", mean, (M, N + 1, 2 * D)), _dev_arg("init", init, (M, N + 1, 2 * D))]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_seed_restarts_dev(self.h.ptr, M, int(seed), int(first), float(scale),
                                                                 int(bool(keep_first)), *args, C.c_void_p(stream or 0)))

    def optimize_queue_seeded(self, seed, start_conf, start_vel, end_conf, end_vel, mean=None, first=0, scale=1.0,
                              keep_first=False, want_init=False):
        """optimize_queue on M restarts made on the device (seed_restarts followed by optimize_queue, without the inits
        crossing to the host): the result() dict with M rows, plus `init` when want_init."""
        D, N = self.D, self.N
        rows = [f64(x).reshape(-1, D) for x in (start_conf, start_vel, end_conf, end_vel)]
        M, sc, ec, mu = seed_inputs(D, N, rows[0], rows[2], mean)
        if any(x.shape[0] != M for x in rows):
            raise ValueError(f"queue inputs disagree on the number of problems: {[x.shape[0] for x in rows]}")
        traj = np.zeros((M, N + 1, 2 * D))
        iters, status = np.zeros(M, dtype=np.int32), np.zeros(M, dtype=np.int32)
        ferr, trace = np.zeros(M), np.zeros((M, self.setting.max_iter + 1))
        init = np.zeros((M, N + 1, 2 * D)) if want_init else None
        self.eng._ck(self.eng.lib.gpmp2mi_plan_optimize_queue_seeded(
            self.h.ptr, M, int(seed), int(first), float(scale), int(bool(keep_first)), dptr(sc), dptr(rows[1]), dptr(ec),
            dptr(rows[3]), dptr(mu), dptr(traj), iptr(iters), dptr(ferr), iptr(status), dptr(trace), dptr(init)))
        out = dict(traj=traj, iters=iters, final_error=ferr, status=status, error_trace=trace)
        if want_init:
            out["init"] = init
        return out

    def optimize_queue_seeded_dev(self, M, seed, start_conf, start_vel, end_conf, end_vel, mean=None, traj=None,
                                  iters=None, final_error=None, status=None, error_trace=None, init_out=None, first=0,
                                  scale=1.0, keep_first=False, stream=None):
        """The same on device buffers (torch tensors or raw pointers); outputs and mean may be None."""
        D, N, T, M = self.D, self.N, self.setting.max_iter + 1, int(M)
        if M < 1:
            raise ValueError("M must be >= 1")
        if any(x is None for x in (start_conf, start_vel, end_conf, end_vel)):
            raise ValueError("start_conf, start_vel, end_conf and end_vel are required")
        t = (M, N + 1, 2 * D)
        args = [_dev_arg("start_conf", start_conf, (M, D)), _dev_arg("start_vel", start_vel, (M, D)),
                _dev_arg("end_conf", end_conf, (M, D)), _dev_arg("end_vel", end_vel, (M, D)), _dev_arg("mean", mean, t),
                _dev_arg("traj", traj, t), _dev_arg("iters", iters, (M,), True),
                _dev_arg("final_error", final_error, (M,)), _dev_arg("status", status, (M,), True),
                _dev_arg("error_trace", error_trace, (M, T)), _dev_arg("init_out", init_out, t)]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_optimize_queue_seeded_dev(
            self.h.ptr, M, int(seed), int(first), float(scale), int(bool(keep_first)), *args, C.c_void_p(stream or 0)))

    def seed_prior(self):
        """(Hdiag [N+1][2D][2D], Hoff [N][2D][2D] = block (i+1, i)): the precision H_seed the restarts are drawn from
        (gpmp2mi_debug_plan_seed_prior)."""
        n, nb = 2 * self.D, self.N + 1
        Hd, Ho = np.zeros((nb, n, n)), np.zeros((nb - 1, n, n))
        self.eng._ck(self.eng.lib.gpmp2mi_debug_plan_seed_prior(self.h.ptr, dptr(Hd), dptr(Ho)))
        return Hd, Ho

    def queue_stats(self):
        """of the last queue run: passes, slot_passes (B * passes), busy_slot_passes (slots that held a problem)."""
        st = _capi.QueueStats()
        self.eng._ck(self.eng.lib.gpmp2mi_plan_queue_stats(self.h.ptr, C.byref(st)))
        return dict(passes=st.passes, slot_passes=st.slot_passes, busy_slot_passes=st.busy_slot_passes)

    def traj_dev_ptr(self):
        return int(self.eng.lib.gpmp2mi_plan_traj_dev(self.h.ptr))

    # ---- scoring and selection of the resident result (include/gpmp2mi.h "scoring")
    def score(self, inter_step, out=None):
        """dict(support_cost, dense_cost, min_clearance, worst, out_of_range) of the plan's result, B rows."""
        inter_step = _score_args(inter_step)
        o = scoring.score_outputs(self.B, out)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_score(self.h.ptr, inter_step, *_score_ptrs(o)))
        return o

    def score_dev(self, inter_step, support_cost=None, dense_cost=None, min_clearance=None, worst=None,
                  out_of_range=None, stream=None):
        """The same into device buffers (torch tensors or raw pointers, any may be None); no host synchronisation."""
        B = self.B
        args = [_dev_arg("support_cost", support_cost, (B,)), _dev_arg("dense_cost", dense_cost, (B,)),
                _dev_arg("min_clearance", min_clearance, (B,)), _dev_arg("worst", worst, (B, 2), True),
                _dev_arg("out_of_range", out_of_range, (B,), True)]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_score_dev(self.h.ptr, _score_args(inter_step), *args,
                                                         C.c_void_p(stream or 0)))

    def select(self, inter_step, required_clearance=0.0, require_in_range=False):
        """Score, apply the rule to the plan's final_error / status, fetch the chosen row: dict(best, n_eligible,
        traj_best [N+1][2D], dense_best [Md][2D]); best = -1: the two trajectories are None."""
        inter_step = _score_args(inter_step)
        Md = scoring.checked_states(self.N, inter_step)
        tb, db = np.zeros((self.N + 1, 2 * self.D)), np.zeros((Md, 2 * self.D))
        best, n = C.c_int(-1), C.c_int(0)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_select(self.h.ptr, inter_step, float(required_clearance),
                                                      int(bool(require_in_range)), C.byref(best), C.byref(n), dptr(tb),
                                                      dptr(db)))
        hit = best.value >= 0
        return dict(best=best.value, n_eligible=n.value, traj_best=tb if hit else None, dense_best=db if hit else None)

    def select_dev(self, inter_step, required_clearance=0.0, require_in_range=False, best=None, n_eligible=None,
                   traj_best=None, dense_best=None, stream=None):
        """The same with device outputs: best / n_eligible int32 [1], traj_best [N+1][2D], dense_best [Md][2D] (torch
        tensors or raw pointers, any may be None).  One enqueue on `stream`, no host synchronisation."""
        inter_step = _score_args(inter_step)
        Md = scoring.checked_states(self.N, inter_step)
        args = [_dev_arg("best", best, (1,), True), _dev_arg("n_eligible", n_eligible, (1,), True),
                _dev_arg("traj_best", traj_best, (self.N + 1, 2 * self.D)),
                _dev_arg("dense_best", dense_best, (Md, 2 * self.D))]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_select_dev(self.h.ptr, inter_step, float(required_clearance),
                                                          int(bool(require_in_range)), *args, C.c_void_p(stream or 0)))

    # ---- the same against the robot itself (include/gpmp2mi.h "self-collision check")
    def self_score(self, pairs, inter_step, out=None):
        """dict(self_support_cost, self_dense_cost, min_self_clearance, worst, invalid) of the plan's result, B rows."""
        inter_step = _score_args(inter_step)
        o = scoring.score_outputs(self.B, out, scoring.SELF_NAMES)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_self_score(self.h.ptr, pairs.ptr, inter_step, *_self_ptrs(o)))
        return o

    def self_score_dev(self, pairs, inter_step, self_support_cost=None, self_dense_cost=None, min_self_clearance=None,
                       worst=None, invalid=None, stream=None):
        """The same into device buffers (torch tensors or raw pointers, any may be None); no host synchronisation."""
        B = self.B
        args = [_dev_arg("self_support_cost", self_support_cost, (B,)), _dev_arg("self_dense_cost", self_dense_cost, (B,)),
                _dev_arg("min_self_clearance", min_self_clearance, (B,)), _dev_arg("worst", worst, (B, 2), True),
                _dev_arg("invalid", invalid, (B,), True)]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_self_score_dev(self.h.ptr, pairs.ptr, _score_args(inter_step), *args,
                                                              C.c_void_p(stream or 0)))

    def select_checked(self, inter_step, pairs, required_clearance=0.0, require_in_range=False,
                       required_self_clearance=0.0):
        """select() with the rule that also asks for required_self_clearance against the pairs of `pairs` and no invalid
        pair: dict(best, n_eligible, traj_best, dense_best); best = -1: the two trajectories are None."""
        inter_step = _score_args(inter_step)
        Md = scoring.checked_states(self.N, inter_step)
        tb, db = np.zeros((self.N + 1, 2 * self.D)), np.zeros((Md, 2 * self.D))
        best, n = C.c_int(-1), C.c_int(0)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_select_checked(
            self.h.ptr, inter_step, float(required_clearance), int(bool(require_in_range)), pairs.ptr,
            float(required_self_clearance), C.byref(best), C.byref(n), dptr(tb), dptr(db)))
        hit = best.value >= 0
        return dict(best=best.value, n_eligible=n.value, traj_best=tb if hit else None, dense_best=db if hit else None)

    def select_checked_dev(self, inter_step, pairs, required_clearance=0.0, require_in_range=False,
                           required_self_clearance=0.0, best=None, n_eligible=None, traj_best=None, dense_best=None,
                           stream=None):
        """The same with device outputs, as select_dev.  One enqueue on `stream`, no host synchronisation."""
        inter_step = _score_args(inter_step)
        Md = scoring.checked_states(self.N, inter_step)
        args = [_dev_arg("best", best, (1,), True), _dev_arg("n_eligible", n_eligible, (1,), True),
                _dev_arg("traj_best", traj_best, (self.N + 1, 2 * self.D)),
                _dev_arg("dense_best", dense_best, (Md, 2 * self.D))]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_select_checked_dev(
            self.h.ptr, inter_step, float(required_clearance), int(bool(require_in_range)), pairs.ptr,
            float(required_self_clearance), *args, C.c_void_p(stream or 0)))

    # ---- can the robot execute it (include/gpmp2mi.h "motion limits")
    def motion_score(self, limits, inter_step, out=None):
        """dict(pos_margin, vel_ratio, acc_ratio, point_speed, time_scale, worst, invalid) of the plan's result, B rows."""
        inter_step = _score_args(inter_step)
        o = scoring.motion_outputs(self.B, out)
        lim = _limits_arg(limits, self.D)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_motion_score(self.h.ptr, lim, inter_step, *_motion_ptrs(o)))
        return o

    def motion_score_dev(self, limits, inter_step, pos_margin=None, vel_ratio=None, acc_ratio=None, point_speed=None,
                         time_scale=None, worst=None, invalid=None, stream=None):
        """The same into device buffers (torch tensors or raw pointers, any may be None); no host synchronisation."""
        B = self.B
        args = [_dev_arg("pos_margin", pos_margin, (B,)), _dev_arg("vel_ratio", vel_ratio, (B,)),
                _dev_arg("acc_ratio", acc_ratio, (B,)), _dev_arg("point_speed", point_speed, (B,)),
                _dev_arg("time_scale", time_scale, (B,)), _dev_arg("worst", worst, (B, 4, 2), True),
                _dev_arg("invalid", invalid, (B,), True)]
        lim, inter_step = _limits_arg(limits, self.D), _score_args(inter_step)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_motion_score_dev(self.h.ptr, lim, inter_step, *args,
                                                                C.c_void_p(stream or 0)))

    def select_feasible(self, inter_step, limits, required_pos_margin=0.0, max_time_scale=1.0, required_clearance=0.0,
                        require_in_range=False, pairs=None, required_self_clearance=0.0):
        """select() (select_checked() when `pairs` is given) with the rule that also asks for no non-finite motion
        quantity, pos_margin >= required_pos_margin and time_scale <= max_time_scale against `limits`:
        dict(best, n_eligible, time_scale_best, traj_best, dense_best); best = -1: the last three are None.  dense_best
        is as planned: divide its velocities by time_scale_best when the row is run that much slower."""
        inter_step = _score_args(inter_step)
        rpm, mts = scoring.feasible_thresholds(required_pos_margin, max_time_scale)
        lim = _limits_arg(limits, self.D)
        Md = scoring.checked_states(self.N, inter_step)
        tb, db = np.zeros((self.N + 1, 2 * self.D)), np.zeros((Md, 2 * self.D))
        best, n, ts = C.c_int(-1), C.c_int(0), C.c_double(0.0)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_select_feasible(
            self.h.ptr, inter_step, float(required_clearance), int(bool(require_in_range)),
            None if pairs is None else pairs.ptr, float(required_self_clearance), lim, rpm, mts,
            C.byref(best), C.byref(n), C.cast(C.byref(ts), _capi.c_double_p), dptr(tb), dptr(db)))
        hit = best.value >= 0
        return dict(best=best.value, n_eligible=n.value, time_scale_best=ts.value if hit else None,
                    traj_best=tb if hit else None, dense_best=db if hit else None)

    def select_feasible_dev(self, inter_step, limits, required_pos_margin=0.0, max_time_scale=1.0, required_clearance=0.0,
                            require_in_range=False, pairs=None, required_self_clearance=0.0, best=None, n_eligible=None,
                            time_scale_best=None, traj_best=None, dense_best=None, stream=None):
        """The same with device outputs, as select_dev, plus time_scale_best float64 [1].  One enqueue on `stream`, no
        host synchronisation once the plan's workspaces hold the shape."""
        inter_step = _score_args(inter_step)
        rpm, mts = scoring.feasible_thresholds(required_pos_margin, max_time_scale)
        lim = _limits_arg(limits, self.D)
        Md = scoring.checked_states(self.N, inter_step)
        args = [_dev_arg("best", best, (1,), True), _dev_arg("n_eligible", n_eligible, (1,), True),
                _dev_arg("time_scale_best", time_scale_best, (1,)),
                _dev_arg("traj_best", traj_best, (self.N + 1, 2 * self.D)),
                _dev_arg("dense_best", dense_best, (Md, 2 * self.D))]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_select_feasible_dev(
            self.h.ptr, inter_step, float(required_clearance), int(bool(require_in_range)),
            None if pairs is None else pairs.ptr, float(required_self_clearance), lim, rpm, mts,
            *args, C.c_void_p(stream or 0)))

    # ---- can the drives produce it (include/gpmp2mi.h "torque limits")
    def torque_score(self, dynamics, inter_step, out=None, tau=True):
        """dict(torque_ratio, static_ratio, torque_time_scale, worst, invalid, tau) of the plan's result, B rows."""
        inter_step = _score_args(inter_step)
        o = scoring.torque_outputs(self.B, scoring.checked_states(self.N, inter_step), self.D, out, tau)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_torque_score(self.h.ptr, dynamics.ptr, inter_step, *_torque_ptrs(o)))
        return o

    def torque_score_dev(self, dynamics, inter_step, torque_ratio=None, static_ratio=None, torque_time_scale=None,
                         worst=None, invalid=None, tau=None, stream=None):
        """The same into device buffers (torch tensors or raw pointers, any may be None); no host synchronisation."""
        inter_step = _score_args(inter_step)
        B, Md = self.B, scoring.checked_states(self.N, inter_step)
        args = [_dev_arg("torque_ratio", torque_ratio, (B,)), _dev_arg("static_ratio", static_ratio, (B,)),
                _dev_arg("torque_time_scale", torque_time_scale, (B,)), _dev_arg("worst", worst, (B, 3, 2), True),
                _dev_arg("invalid", invalid, (B,), True), _dev_arg("tau", tau, (B, Md, self.D))]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_torque_score_dev(self.h.ptr, dynamics.ptr, inter_step, *args,
                                                                C.c_void_p(stream or 0)))

    def select_dynamic(self, inter_step, limits, dynamics, required_pos_margin=0.0, max_time_scale=1.0,
                       required_clearance=0.0, require_in_range=False, pairs=None, required_self_clearance=0.0):
        """select_feasible() with max(time_scale, torque_time_scale) <= max_time_scale in place of its time-scale test
        and no non-finite torque: dict(best, n_eligible, time_scale_best, tau_best, traj_best, dense_best); best = -1:
        the last four are None.  time_scale_best is that maximum; tau_best [Md][D] are the torques at planned timing."""
        inter_step = _score_args(inter_step)
        rpm, mts = scoring.feasible_thresholds(required_pos_margin, max_time_scale)
        lim = _limits_arg(limits, self.D)
        Md = scoring.checked_states(self.N, inter_step)
        tb, db, ub = np.zeros((self.N + 1, 2 * self.D)), np.zeros((Md, 2 * self.D)), np.zeros((Md, self.D))
        best, n, ts = C.c_int(-1), C.c_int(0), C.c_double(0.0)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_select_dynamic(
            self.h.ptr, inter_step, float(required_clearance), int(bool(require_in_range)),
            None if pairs is None else pairs.ptr, float(required_self_clearance), lim, rpm, mts, dynamics.ptr,
            C.byref(best), C.byref(n), C.cast(C.byref(ts), _capi.c_double_p), dptr(ub), dptr(tb), dptr(db)))
        hit = best.value >= 0
        return dict(best=best.value, n_eligible=n.value, time_scale_best=ts.value if hit else None,
                    tau_best=ub if hit else None, traj_best=tb if hit else None, dense_best=db if hit else None)

    def select_dynamic_dev(self, inter_step, limits, dynamics, required_pos_margin=0.0, max_time_scale=1.0,
                           required_clearance=0.0, require_in_range=False, pairs=None, required_self_clearance=0.0,
                           best=None, n_eligible=None, time_scale_best=None, tau_best=None, traj_best=None,
                           dense_best=None, stream=None):
        """The same with device outputs, as select_feasible_dev, plus tau_best float64 [Md][D].  One enqueue on `stream`,
        no host synchronisation once the plan's workspaces hold the shape."""
        inter_step = _score_args(inter_step)
        rpm, mts = scoring.feasible_thresholds(required_pos_margin, max_time_scale)
        lim = _limits_arg(limits, self.D)
        Md = scoring.checked_states(self.N, inter_step)
        args = [_dev_arg("best", best, (1,), True), _dev_arg("n_eligible", n_eligible, (1,), True),
                _dev_arg("time_scale_best", time_scale_best, (1,)), _dev_arg("tau_best", tau_best, (Md, self.D)),
                _dev_arg("traj_best", traj_best, (self.N + 1, 2 * self.D)),
                _dev_arg("dense_best", dense_best, (Md, 2 * self.D))]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_select_dynamic_dev(
            self.h.ptr, inter_step, float(required_clearance), int(bool(require_in_range)),
            None if pairs is None else pairs.ptr, float(required_self_clearance), lim, rpm, mts, dynamics.ptr,
            *args, C.c_void_p(stream or 0)))

    # ---- how fast can the robot run it (include/gpmp2mi.h "re-timing")
    def retime(self, limits, inter_step, max_rate=1.0, rate_start=None, rate_end=None, out=None):
        """dict(sdot, u, stamps, duration, status, achieved, dense_retimed) of the plan's result, B rows."""
        inter_step = _score_args(inter_step)
        rates = scoring.retime_rates(max_rate, rate_start, rate_end)
        o = scoring.retime_outputs(self.B, scoring.checked_states(self.N, inter_step), self.D, out)
        lim = _limits_arg(limits, self.D)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_retime(self.h.ptr, lim, inter_step, *rates, *_retime_ptrs(o)))
        return o

    def retime_dev(self, limits, inter_step, max_rate=1.0, rate_start=None, rate_end=None, sdot=None, u=None,
                   stamps=None, duration=None, status=None, achieved=None, dense_retimed=None, stream=None):
        """The same into device buffers (torch tensors or raw pointers, any may be None); no host synchronisation."""
        inter_step = _score_args(inter_step)
        B, Md = self.B, scoring.checked_states(self.N, inter_step)
        rates = scoring.retime_rates(max_rate, rate_start, rate_end)
        args = [_dev_arg("sdot", sdot, (B, Md)), _dev_arg("u", u, (B, Md)), _dev_arg("stamps", stamps, (B, Md)),
                _dev_arg("duration", duration, (B,)), _dev_arg("status", status, (B,), True),
                _dev_arg("achieved", achieved, (B, 4)), _dev_arg("dense_retimed", dense_retimed, (B, Md, 2 * self.D))]
        lim = _limits_arg(limits, self.D)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_retime_dev(self.h.ptr, lim, inter_step, *rates, *args,
                                                          C.c_void_p(stream or 0)))

    def select_retimed(self, inter_step, limits, required_pos_margin=0.0, max_duration=np.inf, max_rate=1.0,
                       rate_start=None, rate_end=None, required_clearance=0.0, require_in_range=False, pairs=None,
                       required_self_clearance=0.0):
        """select_feasible() with the duration of the re-timed row in place of time_scale: the row must re-time OK within
        max_duration.  dict(best, n_eligible, duration_best, stamps_best, traj_best, dense_best); best = -1: the last
        four are None.  dense_best carries the re-timed velocities (as dense_retimed of retime())."""
        inter_step = _score_args(inter_step)
        rpm, md = scoring.retimed_thresholds(required_pos_margin, max_duration)
        rates = scoring.retime_rates(max_rate, rate_start, rate_end)
        lim = _limits_arg(limits, self.D)
        Md = scoring.checked_states(self.N, inter_step)
        tb, db, sb = np.zeros((self.N + 1, 2 * self.D)), np.zeros((Md, 2 * self.D)), np.zeros(Md)
        best, n, dur = C.c_int(-1), C.c_int(0), C.c_double(0.0)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_select_retimed(
            self.h.ptr, inter_step, float(required_clearance), int(bool(require_in_range)),
            None if pairs is None else pairs.ptr, float(required_self_clearance), lim, rpm, *rates, md,
            C.byref(best), C.byref(n), C.cast(C.byref(dur), _capi.c_double_p), dptr(sb), dptr(tb), dptr(db)))
        hit = best.value >= 0
        return dict(best=best.value, n_eligible=n.value, duration_best=dur.value if hit else None,
                    stamps_best=sb if hit else None, traj_best=tb if hit else None, dense_best=db if hit else None)

    def select_retimed_dev(self, inter_step, limits, required_pos_margin=0.0, max_duration=np.inf, max_rate=1.0,
                           rate_start=None, rate_end=None, required_clearance=0.0, require_in_range=False, pairs=None,
                           required_self_clearance=0.0, best=None, n_eligible=None, duration_best=None,
                           stamps_best=None, traj_best=None, dense_best=None, stream=None):
        """The same with device outputs, as select_feasible_dev, plus duration_best float64 [1] and stamps_best [Md].
        One enqueue on `stream`, no host synchronisation once the plan's workspaces hold the shape."""
        inter_step = _score_args(inter_step)
        rpm, md = scoring.retimed_thresholds(required_pos_margin, max_duration)
        rates = scoring.retime_rates(max_rate, rate_start, rate_end)
        lim = _limits_arg(limits, self.D)
        Md = scoring.checked_states(self.N, inter_step)
        args = [_dev_arg("best", best, (1,), True), _dev_arg("n_eligible", n_eligible, (1,), True),
                _dev_arg("duration_best", duration_best, (1,)), _dev_arg("stamps_best", stamps_best, (Md,)),
                _dev_arg("traj_best", traj_best, (self.N + 1, 2 * self.D)),
                _dev_arg("dense_best", dense_best, (Md, 2 * self.D))]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_select_retimed_dev(
            self.h.ptr, inter_step, float(required_clearance), int(bool(require_in_range)),
            None if pairs is None else pairs.ptr, float(required_self_clearance), lim, rpm, *rates, md,
            *args, C.c_void_p(stream or 0)))

    # ---- a pair table of any size as a factor (include/gpmp2mi.h "self-collision table in a plan")
    def set_self_pairs(self, pairs):
        """The plan's self-collision table: a handle of Engine.self_pairs / generate_self_pairs, whose epsilon and sigma
        columns are the factor's; None or an empty table clears it.  May be repeated between solves; the plan keeps its
        own copy, and must have been created with room for the rows (TrajOptimizerSetting.set_self_pairs)."""
        self.eng._ck(self.eng.lib.gpmp2mi_plan_set_self_pairs(self.h.ptr, None if pairs is None else pairs.ptr))

    def self_pairs_count(self):
        """rows of the table resident in the plan"""
        return int(self.eng.lib.gpmp2mi_plan_self_pairs_count(self.h.ptr))

    # ---- spheres that move with the support time (include/gpmp2mi.h "moving obstacles")
    def set_moving_spheres(self, radius, centers):
        """The plan's sphere set: radius [K], centers [K][N+1][3]; None / empty clears it.  May be repeated between
        solves; the plan must have been created with room for K (TrajOptimizerSetting.set_moving_spheres)."""
        K, r, c = scoring.moving_set(radius, centers, self.N + 1)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_set_moving_spheres(self.h.ptr, K, dptr(r), dptr(c)))

    def set_moving_spheres_dev(self, K, radius, centers, stream=None):
        """The same from device buffers (torch tensors or raw pointers); the copies are enqueued on `stream`."""
        K = int(K)
        args = [_dev_arg("radius", radius, (K,)), _dev_arg("centers", centers, (K, self.N + 1, 3))]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_set_moving_spheres_dev(self.h.ptr, K, *args, C.c_void_p(stream or 0)))

    def moving_score(self, inter_step, out=None):
        """dict(moving_support_cost, moving_dense_cost, min_moving_clearance, worst [B][3], invalid) of the plan's result
        against its resident sphere set, B rows."""
        inter_step = _score_args(inter_step)
        o = scoring.score_outputs(self.B, out, scoring.MOVING_NAMES)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_moving_score(self.h.ptr, inter_step, *_moving_ptrs(o)))
        return o

    def moving_score_dev(self, inter_step, moving_support_cost=None, moving_dense_cost=None, min_moving_clearance=None,
                         worst=None, invalid=None, stream=None):
        """The same into device buffers (torch tensors or raw pointers, any may be None); no host synchronisation."""
        B = self.B
        args = [_dev_arg("moving_support_cost", moving_support_cost, (B,)),
                _dev_arg("moving_dense_cost", moving_dense_cost, (B,)),
                _dev_arg("min_moving_clearance", min_moving_clearance, (B,)), _dev_arg("worst", worst, (B, 3), True),
                _dev_arg("invalid", invalid, (B,), True)]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_moving_score_dev(self.h.ptr, _score_args(inter_step), *args,
                                                                C.c_void_p(stream or 0)))

    def select_moving(self, inter_step, required_moving_clearance=0.0, required_clearance=0.0, require_in_range=False,
                      pairs=None, required_self_clearance=0.0):
        """select() (select_checked() when `pairs` is given) with the rule that also asks for no invalid pair and
        required_moving_clearance against the plan's sphere set: dict(best, n_eligible, traj_best, dense_best);
        best = -1: the two trajectories are None."""
        inter_step = _score_args(inter_step)
        Md = scoring.checked_states(self.N, inter_step)
        tb, db = np.zeros((self.N + 1, 2 * self.D)), np.zeros((Md, 2 * self.D))
        best, n = C.c_int(-1), C.c_int(0)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_select_moving(
            self.h.ptr, inter_step, float(required_clearance), int(bool(require_in_range)),
            None if pairs is None else pairs.ptr, float(required_self_clearance), float(required_moving_clearance),
            C.byref(best), C.byref(n), dptr(tb), dptr(db)))
        hit = best.value >= 0
        return dict(best=best.value, n_eligible=n.value, traj_best=tb if hit else None, dense_best=db if hit else None)

    def select_moving_dev(self, inter_step, required_moving_clearance=0.0, required_clearance=0.0, require_in_range=False,
                          pairs=None, required_self_clearance=0.0, best=None, n_eligible=None, traj_best=None,
                          dense_best=None, stream=None):
        """The same with device outputs, as select_dev.  One enqueue on `stream`, no host synchronisation once the
        plan's workspaces hold the shape."""
        inter_step = _score_args(inter_step)
        Md = scoring.checked_states(self.N, inter_step)
        args = [_dev_arg("best", best, (1,), True), _dev_arg("n_eligible", n_eligible, (1,), True),
                _dev_arg("traj_best", traj_best, (self.N + 1, 2 * self.D)),
                _dev_arg("dense_best", dense_best, (Md, 2 * self.D))]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_select_moving_dev(
            self.h.ptr, inter_step, float(required_clearance), int(bool(require_in_range)),
            None if pairs is None else pairs.ptr, float(required_self_clearance), float(required_moving_clearance),
            *args, C.c_void_p(stream or 0)))

    # ---- one target pose per support state (include/gpmp2mi.h "workspace path")
    def set_workspace_path(self, des, sigma=None):
        """The plan's path: des [N+1][4][4], sigma [N+1] (or a scalar; +inf: the state carries no factor); des None
        clears it.  May be repeated between solves; the plan must have been created with room for a path
        (TrajOptimizerSetting.set_workspace_path)."""
        if des is None:
            self.eng._ck(self.eng.lib.gpmp2mi_plan_set_workspace_path(self.h.ptr, None, None))
            return
        d, s = scoring.path_arrays(des, sigma, self.N + 1)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_set_workspace_path(self.h.ptr, dptr(d), dptr(s)))

    def set_workspace_path_dev(self, des, sigma, stream=None):
        """The same from device buffers (torch tensors or raw pointers); the copies are enqueued on `stream`."""
        args = [_dev_arg("des", des, (self.N + 1, 4, 4)), _dev_arg("sigma", sigma, (self.N + 1,))]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_set_workspace_path_dev(self.h.ptr, *args, C.c_void_p(stream or 0)))

    def path_score(self, inter_step, out=None):
        """dict(max_pos_dev, max_rot_dev, worst [B][2], support_cost, dense_cost, invalid) of the plan's result against
        its resident path, B rows."""
        inter_step = _score_args(inter_step)
        o = scoring.path_outputs(self.B, out)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_path_score(self.h.ptr, inter_step, *_path_ptrs(o)))
        return o

    def path_score_dev(self, inter_step, max_pos_dev=None, max_rot_dev=None, worst=None, support_cost=None,
                       dense_cost=None, invalid=None, stream=None):
        """The same into device buffers (torch tensors or raw pointers, any may be None); no host synchronisation."""
        B = self.B
        args = [_dev_arg("max_pos_dev", max_pos_dev, (B,)), _dev_arg("max_rot_dev", max_rot_dev, (B,)),
                _dev_arg("worst", worst, (B, 2), True), _dev_arg("support_cost", support_cost, (B,)),
                _dev_arg("dense_cost", dense_cost, (B,)), _dev_arg("invalid", invalid, (B,), True)]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_path_score_dev(self.h.ptr, _score_args(inter_step), *args,
                                                              C.c_void_p(stream or 0)))

    def select_path(self, inter_step, max_pos_dev_allowed=np.inf, max_rot_dev_allowed=np.inf, required_clearance=0.0,
                    require_in_range=False):
        """select() with the rule that also asks for no invalid checked state and deviations from the plan's path
        within the two allowances: dict(best, n_eligible, traj_best, dense_best); best = -1: the two trajectories
        are None."""
        inter_step = _score_args(inter_step)
        Md = scoring.checked_states(self.N, inter_step)
        tb, db = np.zeros((self.N + 1, 2 * self.D)), np.zeros((Md, 2 * self.D))
        best, n = C.c_int(-1), C.c_int(0)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_select_path(
            self.h.ptr, inter_step, float(required_clearance), int(bool(require_in_range)), float(max_pos_dev_allowed),
            float(max_rot_dev_allowed), C.byref(best), C.byref(n), dptr(tb), dptr(db)))
        hit = best.value >= 0
        return dict(best=best.value, n_eligible=n.value, traj_best=tb if hit else None, dense_best=db if hit else None)

    def select_path_dev(self, inter_step, max_pos_dev_allowed=np.inf, max_rot_dev_allowed=np.inf, required_clearance=0.0,
                        require_in_range=False, best=None, n_eligible=None, traj_best=None, dense_best=None, stream=None):
        """The same with device outputs, as select_dev.  One enqueue on `stream`, no host synchronisation once the
        plan's workspaces hold the shape."""
        inter_step = _score_args(inter_step)
        Md = scoring.checked_states(self.N, inter_step)
        args = [_dev_arg("best", best, (1,), True), _dev_arg("n_eligible", n_eligible, (1,), True),
                _dev_arg("traj_best", traj_best, (self.N + 1, 2 * self.D)),
                _dev_arg("dense_best", dense_best, (Md, 2 * self.D))]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_select_path_dev(
            self.h.ptr, inter_step, float(required_clearance), int(bool(require_in_range)), float(max_pos_dev_allowed),
            float(max_rot_dev_allowed), *args, C.c_void_p(stream or 0)))

    # ---- one representative per mode of the resident result (include/gpmp2mi.h "distinct alternatives")
    def _distinct_args(self, inter_step, radius, weights, metric, max_alt):
        max_alt = int(max_alt)
        if not 1 <= max_alt <= scoring.MAX_ALTERNATIVES:
            raise ValueError(f"max_alt must be in 1..{scoring.MAX_ALTERNATIVES}")
        if self.B > scoring.MAX_GROUP_ROWS:
            raise ValueError(f"at most {scoring.MAX_GROUP_ROWS} rows can be grouped, got {self.B}")
        return (_score_args(inter_step), scoring.group_radius(radius), scoring.group_weights(weights, self.D),
                scoring.group_metric(metric), max_alt)

    def select_distinct(self, inter_step, radius, max_alt=8, required_clearance=0.0, require_in_range=False, pairs=None,
                        required_self_clearance=0.0, weights=None, metric=scoring.DIST_MAX_STATE, fill=np.nan):
        """Score, apply the rule of select() (of select_checked() when `pairs` is given), group the eligible rows by the
        leader rule with final_error as the score, fetch one row per mode: dict(n_modes, n_eligible, alt [max_alt],
        alt_size [max_alt], alt_error [max_alt], mode [B], traj_alt [max_alt][N+1][2D], dense_alt [max_alt][Md][2D]).
        n_modes counts all modes; entries beyond min(n_modes, max_alt) are -1 / 0 / `fill`."""
        inter_step, radius, w, metric, max_alt = self._distinct_args(inter_step, radius, weights, metric, max_alt)
        Md = scoring.checked_states(self.N, inter_step)
        nm, ne = C.c_int(0), C.c_int(0)
        alt, size = np.full(max_alt, -1, dtype=np.int32), np.zeros(max_alt, dtype=np.int32)
        err, mode = np.full(max_alt, float(fill)), np.full(self.B, -1, dtype=np.int32)
        ta = np.full((max_alt, self.N + 1, 2 * self.D), float(fill))
        da = np.full((max_alt, Md, 2 * self.D), float(fill))
        self.eng._ck(self.eng.lib.gpmp2mi_plan_select_distinct(
            self.h.ptr, inter_step, float(required_clearance), int(bool(require_in_range)),
            None if pairs is None else pairs.ptr, float(required_self_clearance), metric, dptr(w), radius, max_alt,
            C.byref(nm), C.byref(ne), iptr(alt), iptr(size), dptr(err), iptr(mode), dptr(ta), dptr(da)))
        return dict(n_modes=nm.value, n_eligible=ne.value, alt=alt, alt_size=size, alt_error=err, mode=mode, traj_alt=ta,
                    dense_alt=da)

    def select_distinct_dev(self, inter_step, radius, max_alt=8, required_clearance=0.0, require_in_range=False,
                            pairs=None, required_self_clearance=0.0, weights=None, metric=scoring.DIST_MAX_STATE,
                            n_modes=None, n_eligible=None, alt=None, alt_size=None, alt_error=None, mode=None,
                            traj_alt=None, dense_alt=None, stream=None):
        """The same with device outputs (torch tensors or raw pointers, any may be None): n_modes / n_eligible int32 [1],
        alt / alt_size int32 [max_alt], alt_error [max_alt], mode int32 [B], traj_alt [max_alt][N+1][2D], dense_alt
        [max_alt][Md][2D].  weights stays a host array.  One enqueue on `stream`, no host synchronisation."""
        inter_step, radius, w, metric, max_alt = self._distinct_args(inter_step, radius, weights, metric, max_alt)
        Md = scoring.checked_states(self.N, inter_step)
        args = [_dev_arg("n_modes", n_modes, (1,), True), _dev_arg("n_eligible", n_eligible, (1,), True),
                _dev_arg("alt", alt, (max_alt,), True), _dev_arg("alt_size", alt_size, (max_alt,), True),
                _dev_arg("alt_error", alt_error, (max_alt,)), _dev_arg("mode", mode, (self.B,), True),
                _dev_arg("traj_alt", traj_alt, (max_alt, self.N + 1, 2 * self.D)),
                _dev_arg("dense_alt", dense_alt, (max_alt, Md, 2 * self.D))]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_select_distinct_dev(
            self.h.ptr, inter_step, float(required_clearance), int(bool(require_in_range)),
            None if pairs is None else pairs.ptr, float(required_self_clearance), metric, dptr(w), radius, max_alt,
            *args, C.c_void_p(stream or 0)))

    def graph_error(self, traj):
        t = f64(traj).reshape(self.B, self.N + 1, 2 * self.D)
        err = np.zeros(self.B)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_graph_error(self.h.ptr, dptr(t), dptr(err)))
        return err

    def linearize(self, traj):
        B, n, nb = self.B, 2 * self.D, self.N + 1
        t = f64(traj).reshape(B, nb, n)
        Hd, Ho = np.zeros((B, nb, n, n)), np.zeros((B, nb - 1, n, n))
        g, err = np.zeros((B, nb, n)), np.zeros(B)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_linearize(self.h.ptr, dptr(t), dptr(Hd), dptr(Ho), dptr(g), dptr(err)))
        return Hd, Ho, g, err

    # ---- the posterior at the estimate (include/gpmp2mi.h "posterior")
    def marginals(self, traj=None):
        """Sigma = H^-1 of the plan's graph at `traj` ([B][N+1][2D]; None: the current estimate) ->
        dict(Sdiag [B][N+1][2D][2D], Soff [B][N][2D][2D] = block (i+1, i), ok [B])."""
        B, n, nb = self.B, 2 * self.D, self.N + 1
        t = None if traj is None else f64(traj).reshape(B, nb, n)
        Sd, So, ok = np.zeros((B, nb, n, n)), np.zeros((B, nb - 1, n, n)), np.zeros(B, dtype=np.int32)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_marginals(self.h.ptr, dptr(t), dptr(Sd), dptr(So), iptr(ok)))
        return dict(Sdiag=Sd, Soff=So, ok=ok)

    def marginals_dev(self, Sdiag=None, Soff=None, ok=None, stream=None):
        """The same at the current estimate into device buffers (torch tensors or raw pointers, any may be None); no host
        synchronisation."""
        B, n, nb = self.B, 2 * self.D, self.N + 1
        args = [_dev_arg("Sdiag", Sdiag, (B, nb, n, n)), _dev_arg("Soff", Soff, (B, nb - 1, n, n)),
                _dev_arg("ok", ok, (B,), True)]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_marginals_dev(self.h.ptr, *args, C.c_void_p(stream or 0)))

    # ---- the posterior on the executed timeline (include/gpmp2mi.h)
    def marginals_dense(self, inter_step):
        """The posterior at the current estimate carried to the Md = N (inter_step + 1) + 1 checked states:
        dict(cov [B][Md][2D][2D], ok [B])."""
        inter_step = _score_args(inter_step)
        B, n, Md = self.B, 2 * self.D, scoring.checked_states(self.N, inter_step)
        cov, ok = np.zeros((B, Md, n, n)), np.zeros(B, dtype=np.int32)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_marginals_dense(self.h.ptr, inter_step, dptr(cov), iptr(ok)))
        return dict(cov=cov, ok=ok)

    def marginals_dense_dev(self, inter_step, cov=None, ok=None, stream=None):
        """The same into device buffers (torch tensors or raw pointers, any may be None); no host synchronisation."""
        inter_step = _score_args(inter_step)
        B, n, Md = self.B, 2 * self.D, scoring.checked_states(self.N, inter_step)
        args = [_dev_arg("cov", cov, (B, Md, n, n)), _dev_arg("ok", ok, (B,), True)]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_marginals_dense_dev(self.h.ptr, inter_step, *args,
                                                                   C.c_void_p(stream or 0)))

    def risk(self, inter_step, kappa, want_sigma=True):
        """The k-sigma clearance of the plan's current estimate, B rows: dict(robust_clearance, worst [B][2],
        sigma_worst, out_of_range, sigma [B][Md][S] or None, ok)."""
        inter_step, kappa = _score_args(inter_step), _kappa_arg(kappa)
        B, Md = self.B, scoring.checked_states(self.N, inter_step)
        o = dict(robust_clearance=np.zeros(B), worst=np.zeros((B, 2), dtype=np.int32), sigma_worst=np.zeros(B),
                 out_of_range=np.zeros(B, dtype=np.int32),
                 sigma=np.zeros((B, Md, self.robot.S)) if want_sigma else None, ok=np.zeros(B, dtype=np.int32))
        self.eng._ck(self.eng.lib.gpmp2mi_plan_risk(self.h.ptr, inter_step, kappa, dptr(o["robust_clearance"]),
                                                    iptr(o["worst"]), dptr(o["sigma_worst"]), iptr(o["out_of_range"]),
                                                    dptr(o["sigma"]), iptr(o["ok"])))
        return o

    def risk_dev(self, inter_step, kappa, robust_clearance=None, worst=None, sigma_worst=None, out_of_range=None,
                 sigma=None, ok=None, stream=None):
        """The same into device buffers (torch tensors or raw pointers, any may be None); no host synchronisation."""
        inter_step, kappa = _score_args(inter_step), _kappa_arg(kappa)
        B, Md = self.B, scoring.checked_states(self.N, inter_step)
        args = [_dev_arg("robust_clearance", robust_clearance, (B,)), _dev_arg("worst", worst, (B, 2), True),
                _dev_arg("sigma_worst", sigma_worst, (B,)), _dev_arg("out_of_range", out_of_range, (B,), True),
                _dev_arg("sigma", sigma, (B, Md, self.robot.S)), _dev_arg("ok", ok, (B,), True)]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_risk_dev(self.h.ptr, inter_step, kappa, *args, C.c_void_p(stream or 0)))

    def sample_posterior(self, z):
        """z [B][K][N+1][2D] -> delta of the same shape, delta = L^-T z (H = L L^T at the current estimate): for
        z ~ N(0, I), perturbations of the estimate drawn from the posterior."""
        B, n, nb = self.B, 2 * self.D, self.N + 1
        z = f64(z)
        if z.ndim != 4 or z.shape[0] != B or z.shape[1] < 1 or z.shape[2:] != (nb, n):
            raise ValueError(f"z: expected [{B}][K][{nb}][{n}] with K >= 1, got {list(z.shape)}")
        delta = np.zeros_like(z)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_sample_posterior(self.h.ptr, z.shape[1], dptr(z), dptr(delta), None))
        return delta

    def sample_posterior_dev(self, K, z, delta, ok=None, stream=None):
        """The same on device buffers: z, delta [B][K][N+1][2D], ok int32 [B] or None; no host synchronisation."""
        B, n, nb, K = self.B, 2 * self.D, self.N + 1, int(K)
        if K < 1:
            raise ValueError("K must be >= 1")
        if z is None or delta is None:
            raise ValueError("z and delta are required")
        args = [_dev_arg("z", z, (B, K, nb, n)), _dev_arg("delta", delta, (B, K, nb, n)), _dev_arg("ok", ok, (B,), True)]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_sample_posterior_dev(self.h.ptr, K, *args, C.c_void_p(stream or 0)))

    def sample_posterior_seeded(self, K, seed, row_first=0, sample_first=0):
        """sample_posterior with z made on the device: (delta [B][K][N+1][2D], ok [B]); z of (row b, sample s) is the
        counter RNG at (seed, row_first + b, sample_first + s)."""
        B, n, nb, K = self.B, 2 * self.D, self.N + 1, int(K)
        if K < 1:
            raise ValueError("K must be >= 1")
        delta, ok = np.zeros((B, K, nb, n)), np.zeros(B, dtype=np.int32)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_sample_posterior_seeded(self.h.ptr, K, int(seed), int(row_first),
                                                                       int(sample_first), dptr(delta), iptr(ok)))
        return delta, ok

    def sample_posterior_seeded_dev(self, K, seed, delta, ok=None, row_first=0, sample_first=0, stream=None):
        """The same into device buffers: delta [B][K][N+1][2D], ok int32 [B] or None; no host synchronisation."""
        B, n, nb, K = self.B, 2 * self.D, self.N + 1, int(K)
        if K < 1:
            raise ValueError("K must be >= 1")
        if delta is None:
            raise ValueError("delta is required")
        args = [_dev_arg("delta", delta, (B, K, nb, n)), _dev_arg("ok", ok, (B,), True)]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_sample_posterior_seeded_dev(
            self.h.ptr, K, int(seed), int(row_first), int(sample_first), *args, C.c_void_p(stream or 0)))

    # ---- sampled clearance (include/gpmp2mi.h "sampled clearance")
    def collision_probability(self, inter_step, K, seed, required_clearance=0.0, row_first=0, sample_first=0, bridge=True,
                              want_maps=True):
        """K joint draws of the executed trajectory per row from the posterior at the current estimate, each through the
        collision check: dict(hits [B], probability [B] = hits / K, clearance [B][K], worst [B][K][2],
        state_clearance [B][K][Md] or None, state_hits [B][Md], oor_samples [B], ok [B])."""
        inter_step, K, row_first, sample_first, required_clearance = sampled_args(
            inter_step, K, row_first, sample_first, required_clearance)
        o = sampled_outputs(self.B, K, scoring.checked_states(self.N, inter_step), self.D, want_maps)
        del o["conf"]
        o["ok"] = np.zeros(self.B, dtype=np.int32)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_collision_probability(
            self.h.ptr, inter_step, K, int(seed), row_first, sample_first, int(bool(bridge)), required_clearance,
            *_sampled_ptrs(o), iptr(o["ok"])))
        return o

    def collision_probability_dev(self, inter_step, K, seed, required_clearance=0.0, row_first=0, sample_first=0,
                                  bridge=True, hits=None, probability=None, clearance=None, worst=None,
                                  state_clearance=None, state_hits=None, oor_samples=None, ok=None, stream=None):
        """The same into device buffers (torch tensors or raw pointers, any may be None); no host synchronisation once the
        plan holds the bridge factors of this inter_step."""
        inter_step, K, row_first, sample_first, required_clearance = sampled_args(
            inter_step, K, row_first, sample_first, required_clearance)
        B, Md = self.B, scoring.checked_states(self.N, inter_step)
        args = _sampled_dev_args(B, K, Md, hits, probability, clearance, worst, state_clearance, state_hits, oor_samples)
        args.append(_dev_arg("ok", ok, (B,), True))
        self.eng._ck(self.eng.lib.gpmp2mi_plan_collision_probability_dev(
            self.h.ptr, inter_step, K, int(seed), row_first, sample_first, int(bool(bridge)), required_clearance, *args,
            C.c_void_p(stream or 0)))

    def sample_dense_seeded(self, inter_step, K, seed, row_first=0, sample_first=0, bridge=True):
        """(conf [B][K][Md][D], ok [B]): the sampled configurations on the executed timeline alone."""
        inter_step, K, row_first, sample_first, _ = sampled_args(inter_step, K, row_first, sample_first)
        conf = np.zeros((self.B, K, scoring.checked_states(self.N, inter_step), self.D))
        ok = np.zeros(self.B, dtype=np.int32)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_sample_dense_seeded(
            self.h.ptr, inter_step, K, int(seed), row_first, sample_first, int(bool(bridge)), dptr(conf), iptr(ok)))
        return conf, ok

    def sample_dense_seeded_dev(self, inter_step, K, seed, conf, ok=None, row_first=0, sample_first=0, bridge=True,
                                stream=None):
        """The same into device buffers: conf [B][K][Md][D], ok int32 [B] or None."""
        inter_step, K, row_first, sample_first, _ = sampled_args(inter_step, K, row_first, sample_first)
        if conf is None:
            raise ValueError("conf is required")
        B, Md = self.B, scoring.checked_states(self.N, inter_step)
        args = [_dev_arg("conf", conf, (B, K, Md, self.D)), _dev_arg("ok", ok, (B,), True)]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_sample_dense_seeded_dev(
            self.h.ptr, inter_step, K, int(seed), row_first, sample_first, int(bool(bridge)), *args,
            C.c_void_p(stream or 0)))

    # ---- incremental replanning (ISAM2TrajOptimizer's role; see include/gpmp2mi.h)
    def fix_state(self, b, state_idx, conf, vel):
        c, v = f64(conf).reshape(self.D), f64(vel).reshape(self.D)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_fix_state(self.h.ptr, int(b), int(state_idx), dptr(c), dptr(v)))

    def add_state_estimate(self, b, state_idx, conf, conf_cov, vel=None, vel_cov=None):
        c, cc = f64(conf).reshape(self.D), f64(conf_cov).reshape(self.D, self.D)
        v = None if vel is None else f64(vel).reshape(self.D)
        vc = None if vel_cov is None else f64(vel_cov).reshape(self.D, self.D)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_add_state_estimate(self.h.ptr, int(b), int(state_idx), dptr(c), dptr(cc),
                                                                  dptr(v), dptr(vc)))

    def change_goal(self, b, goal_conf, goal_vel):
        c, v = f64(goal_conf).reshape(self.D), f64(goal_vel).reshape(self.D)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_change_goal(self.h.ptr, int(b), dptr(c), dptr(v)))

    def remove_goal(self, b):
        self.eng._ck(self.eng.lib.gpmp2mi_plan_remove_goal(self.h.ptr, int(b)))

    def clear_state_priors(self, b):
        self.eng._ck(self.eng.lib.gpmp2mi_plan_clear_state_priors(self.h.ptr, int(b)))

    def update(self, iterations=1, stream=None):
        self.eng._ck(self.eng.lib.gpmp2mi_plan_update(self.h.ptr, int(iterations), C.c_void_p(stream or 0)))

    def debug_scalars(self, b):
        out = np.zeros(17)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_debug_scalars(self.h.ptr, int(b), dptr(out)))
        return dict(gd=out[0], dd=out[1], gg=out[2], ghg=out[3], gn=out[4], nn=out[5], q=out[6], xnorm=out[7], radius=out[16])

    def enable_timing(self, on=True):
        self.eng._ck(self.eng.lib.gpmp2mi_plan_enable_timing(self.h.ptr, int(on)))

    def timing(self):
        n = C.c_int(16)
        names = (C.c_char_p * 16)()
        ms = (C.c_double * 16)()
        launches = (C.c_int * 16)()
        self.eng._ck(self.eng.lib.gpmp2mi_plan_get_timing(self.h.ptr, C.byref(n), names, ms, launches))
        return {names[i].decode(): dict(ms=ms[i], launches=launches[i]) for i in range(min(n.value, 16))}


class MultiPlan:
    """gpmp2mi_multi_plan: B trajectory problems sharded over several devices of this process, one plan and one stream
    per entry of `devices` (include/gpmp2mi.h).  Rows are in batch order everywhere; forms / replicate_all (tests): see
    gpmp2mi_debug_multi_plan_create in include/gpmp2mi_debug.h."""

    def __init__(self, eng: Engine, robot, sdf, setting, B, devices, forms=None, replicate_all=False):
        B, devices = multi_plan_args(B, devices)
        self.eng, self.robot, self.sdf, self.setting, self.B = eng, robot, sdf, setting, B
        self.D, self.N, self.T = setting.dof, setting.total_step, setting.max_iter + 1
        s, o, keep = _capi.make_settings(setting)
        self._keep = (s, o, keep)
        devs = np.asarray(devices, dtype=np.int32)
        out = C.c_void_p()
        if forms is None and not replicate_all:
            eng._ck(eng.lib.gpmp2mi_multi_plan_create(robot.ptr, sdf.ptr, C.byref(s), C.byref(o), B, len(devices),
                                                      iptr(devs), C.byref(out)))
        else:
            f = _capi.make_debug_forms(forms or {})
            eng._ck(eng.lib.gpmp2mi_debug_multi_plan_create(robot.ptr, sdf.ptr, C.byref(s), C.byref(o), B, len(devices),
                                                            iptr(devs), C.byref(f), int(bool(replicate_all)),
                                                            C.byref(out)))
        self.h = _Handle(out, eng.lib.gpmp2mi_multi_plan_destroy)

    def close(self):
        self.h.close()

    def shards(self):
        """(devices, row_begin): shard k holds rows row_begin[k] .. row_begin[k + 1] - 1."""
        n = C.c_int()
        devs, rb = np.zeros(_capi.MAX_SHARDS, dtype=np.int32), np.zeros(_capi.MAX_SHARDS + 1, dtype=np.int32)
        self.eng._ck(self.eng.lib.gpmp2mi_multi_plan_shards(self.h.ptr, C.byref(n), iptr(devs), iptr(rb)))
        return [int(x) for x in devs[:n.value]], [int(x) for x in rb[:n.value + 1]]

    def set_problem(self, start_conf, start_vel, end_conf, end_vel, init):
        B, (sc, sv, ec, ev), t = queue_inputs(self.D, self.N, start_conf, start_vel, end_conf, end_vel, init)
        if B != self.B:
            raise ValueError(f"expected {self.B} rows, got {B}")
        self.eng._ck(self.eng.lib.gpmp2mi_multi_plan_set_problem(self.h.ptr, dptr(sc), dptr(sv), dptr(ec), dptr(ev),
                                                                 dptr(t)))

    def refresh_field(self):
        """After an update of the field handle this multi plan was made on (include/gpmp2mi.h "live map"): the new voxels
        to every copy of the field the multi plan owns."""
        self.eng._ck(self.eng.lib.gpmp2mi_multi_plan_refresh_field(self.h.ptr))

    def optimize(self):
        self.eng._ck(self.eng.lib.gpmp2mi_multi_plan_optimize(self.h.ptr))

    def result(self):
        B, D, N = self.B, self.D, self.N
        traj = np.zeros((B, N + 1, 2 * D))
        iters, status = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        ferr, trace = np.zeros(B), np.zeros((B, self.T))
        self.eng._ck(self.eng.lib.gpmp2mi_multi_plan_get_result(self.h.ptr, dptr(traj), iptr(iters), dptr(ferr),
                                                                iptr(status), dptr(trace)))
        return dict(traj=traj, iters=iters, final_error=ferr, status=status, error_trace=trace)

    def result_dev(self, device, traj=None, iters=None, final_error=None, status=None, stream=None):
        """Gather onto `device` (no host synchronisation): torch tensors there (checked for device, dtype, contiguity and
        shape) or raw device pointers (ints); any may be None.  stream: a hipStream_t on `device` as int."""
        B, D, N = self.B, self.D, self.N
        shapes = [(B, N + 1, 2 * D), (B,), (B,), (B,)]
        names, ints = ["traj", "iters", "final_error", "status"], {"iters", "status"}
        args = []
        for name, shape, x in zip(names, shapes, (traj, iters, final_error, status)):
            if x is not None and hasattr(x, "data_ptr"):
                want = "torch.int32" if name in ints else "torch.float64"
                if (str(x.dtype) != want or not x.is_contiguous() or tuple(x.shape) != shape or x.device.type != "cuda"
                        or x.device.index != int(device)):
                    raise ValueError(f"{name}: expected a contiguous {want} tensor of shape {list(shape)} on cuda:{device},"
                                     f" got {x.dtype} {list(x.shape)} on {x.device}")
                x = x.data_ptr()
            args.append(None if x is None else C.c_void_p(int(x)))
        self.eng._ck(self.eng.lib.gpmp2mi_multi_plan_get_result_dev(self.h.ptr, int(device), *args,
                                                                    C.c_void_p(stream or 0)))

    def optimize_queue(self, start_conf, start_vel, end_conf, end_vel, init):
        """M problems (host arrays), split over the shards: the result() dict with M rows, row j = problem j."""
        M, (sc, sv, ec, ev), t = queue_inputs(self.D, self.N, start_conf, start_vel, end_conf, end_vel, init)
        D, N = self.D, self.N
        traj = np.zeros((M, N + 1, 2 * D))
        iters, status = np.zeros(M, dtype=np.int32), np.zeros(M, dtype=np.int32)
        ferr, trace = np.zeros(M), np.zeros((M, self.T))
        self.eng._ck(self.eng.lib.gpmp2mi_multi_plan_optimize_queue(self.h.ptr, M, dptr(sc), dptr(sv), dptr(ec), dptr(ev),
                                                                    dptr(t), dptr(traj), iptr(iters), dptr(ferr),
                                                                    iptr(status), dptr(trace)))
        return dict(traj=traj, iters=iters, final_error=ferr, status=status, error_trace=trace)

    def optimize_queue_seeded(self, seed, start_conf, start_vel, end_conf, end_vel, mean=None, first=0, scale=1.0,
                              keep_first=False, want_init=False):
        """Plan.optimize_queue_seeded split over the shards: the same rows as one plan returns."""
        D, N = self.D, self.N
        rows = [f64(x).reshape(-1, D) for x in (start_conf, start_vel, end_conf, end_vel)]
        M, sc, ec, mu = seed_inputs(D, N, rows[0], rows[2], mean)
        if any(x.shape[0] != M for x in rows):
            raise ValueError(f"queue inputs disagree on the number of problems: {[x.shape[0] for x in rows]}")
        traj = np.zeros((M, N + 1, 2 * D))
        iters, status = np.zeros(M, dtype=np.int32), np.zeros(M, dtype=np.int32)
        ferr, trace = np.zeros(M), np.zeros((M, self.T))
        init = np.zeros((M, N + 1, 2 * D)) if want_init else None
        self.eng._ck(self.eng.lib.gpmp2mi_multi_plan_optimize_queue_seeded(
            self.h.ptr, M, int(seed), int(first), float(scale), int(bool(keep_first)), dptr(sc), dptr(rows[1]), dptr(ec),
            dptr(rows[3]), dptr(mu), dptr(traj), iptr(iters), dptr(ferr), iptr(status), dptr(trace), dptr(init)))
        out = dict(traj=traj, iters=iters, final_error=ferr, status=status, error_trace=trace)
        if want_init:
            out["init"] = init
        return out

    def score(self, inter_step, out=None):
        """Plan.score over all shards, rows in batch order."""
        inter_step = _score_args(inter_step)
        o = scoring.score_outputs(self.B, out)
        self.eng._ck(self.eng.lib.gpmp2mi_multi_plan_score(self.h.ptr, inter_step, *_score_ptrs(o)))
        return o

    def select(self, inter_step, required_clearance=0.0, require_in_range=False):
        """Plan.select over all shards: `best` is a batch row."""
        inter_step = _score_args(inter_step)
        Md = scoring.checked_states(self.N, inter_step)
        tb, db = np.zeros((self.N + 1, 2 * self.D)), np.zeros((Md, 2 * self.D))
        best, n = C.c_int(-1), C.c_int(0)
        self.eng._ck(self.eng.lib.gpmp2mi_multi_plan_select(self.h.ptr, inter_step, float(required_clearance),
                                                            int(bool(require_in_range)), C.byref(best), C.byref(n),
                                                            dptr(tb), dptr(db)))
        hit = best.value >= 0
        return dict(best=best.value, n_eligible=n.value, traj_best=tb if hit else None, dense_best=db if hit else None)

    def queue_stats(self, shard):
        """of the last queue run, shard `shard`: passes, slot_passes, busy_slot_passes (zeros if it had no problems)."""
        st = _capi.QueueStats()
        self.eng._ck(self.eng.lib.gpmp2mi_multi_plan_queue_stats(self.h.ptr, int(shard), C.byref(st)))
        return dict(passes=st.passes, slot_passes=st.slot_passes, busy_slot_passes=st.busy_slot_passes)
