"""ctypes binding of the HIP product library (gpmp2_amd/csrc/libgpmp2mi.so, C ABI of
include/gpmp2mi.h).  There is no Python/CPU compute path here: if the shared library is missing
or no GPU is usable every call raises.

This module loads the library and holds Engine with its core, the factor-level calls, the posterior, seeding and
goal-configuration calls.  The rest of Engine is mixed in by section of the header: the field, map, sensor and scene calls
from fields.py, the checks of host trajectories from checks.py.  Plan and MultiPlan are in plan.py, what they all share
in front of a call in marshalling.py; every name that was importable from here still is."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _capi, scoring
from ._capi import dptr, f64, iptr  # noqa: F401
from .checks import TrajChecks
from .fields import FieldCalls
from .marshalling import (Dynamics, MotionLimits, _dev_arg, _Handle, _kappa_arg, _limits_arg,  # noqa: F401
                          _sampled_dev_args, _sampled_ptrs, _score_args, band_inputs, multi_plan_args, queue_inputs,
                          sampled_args, sampled_outputs, seed_inputs)
from .plan import MultiPlan, Plan

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
    _capi.declare_retime_dynamic(lib)
    _capi.declare_moving(lib)
    _capi.declare_carried(lib)
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


class Engine(FieldCalls, TrajChecks):
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

    def carried_sphere_factor(self, robot, sdf, link, radius, centers, epsilon, conf, jac=True):
        """The carried-object hinge (include/gpmp2mi.h "carried object"): radius [A], centers [A][3] in the frame of
        `link`, conf [M][D] -> err [M][A], H [M][A][D]"""
        q = f64(conf).reshape(-1, robot.dof)
        M = q.shape[0]
        A, r, c = scoring.carried_set(radius, centers)
        err, H = np.zeros((M, A)), (np.zeros((M, A, robot.dof)) if jac else None)
        self._ck(self.lib.gpmp2mi_carried_sphere_factor(robot.ptr, sdf.ptr, int(link), A, dptr(r), dptr(c),
                                                        float(epsilon), M, dptr(q), dptr(err), dptr(H)))
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
