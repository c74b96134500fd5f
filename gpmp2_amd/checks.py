"""The checks of host trajectories of Engine: the seven check stages of stages.py on caller-supplied trajectories, the
host selection rule, the pair tables and the grouping into distinct alternatives (include/gpmp2mi.h "scoring" to
"workspace path" and "distinct alternatives")."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import scoring, stages
from ._capi import dptr, f64, iptr
from .marshalling import Dynamics, _dev_arg, _Handle, _limits_arg, dev_args, out_ptrs, traj_args


class TrajChecks:
    """Mixed into Engine, which brings self.lib and self._ck."""

    # ---------------------------------------------------------------- scoring (include/gpmp2mi.h "scoring")
    def score_traj(self, robot, sdf, delta_t, inter_step, traj, out=None):
        """traj [B][N+1][2D] (or one [N+1][2D]) -> dict(support_cost [B], dense_cost [B], min_clearance [B],
        worst [B][2] = (checked state, sphere), out_of_range [B]) of the inter_step-up-sampled trajectories.
        out: a dict of caller arrays to fill instead (checked).  ValueError for mis-shaped arrays."""
        t, inter_step, delta_t, B, N = traj_args(traj, robot.dof, delta_t, inter_step)
        o = stages.outputs(stages.SCORE, B, out=out)
        self._ck(self.lib.gpmp2mi_score_traj(robot.ptr, sdf.ptr, delta_t, inter_step, B, N, dptr(t),
                                             *out_ptrs(stages.SCORE, o)))
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
        t, inter_step, delta_t, B, N = traj_args(traj, robot.dof, delta_t, inter_step)
        o = stages.outputs(stages.SELF, B, out=out)
        self._ck(self.lib.gpmp2mi_self_score_traj(robot.ptr, pairs.ptr, delta_t, inter_step, B, N, dptr(t),
                                                  *out_ptrs(stages.SELF, o)))
        return o

    # ---------------------------------------------------------------- motion limits (include/gpmp2mi.h)
    def motion_score_traj(self, robot, limits, delta_t, inter_step, traj, out=None):
        """traj [B][N+1][2D] (or one [N+1][2D]) -> dict(pos_margin [B], vel_ratio [B], acc_ratio [B], point_speed [B],
        time_scale [B], worst [B][4][2], invalid [B]) of the inter_step-up-sampled trajectories against `limits` (a
        MotionLimits; None: no limit)."""
        t, inter_step, delta_t, B, N = traj_args(traj, robot.dof, delta_t, inter_step)
        o = stages.outputs(stages.MOTION, B, out=out)
        lim = _limits_arg(limits, robot.dof)
        self._ck(self.lib.gpmp2mi_motion_score_traj(robot.ptr, lim, delta_t, inter_step, B, N, dptr(t),
                                                    *out_ptrs(stages.MOTION, o)))
        return o

    # ---------------------------------------------------------------- torque limits (include/gpmp2mi.h)
    def dynamics(self, robot, mass, com, inertia, gravity=(0.0, 0.0, -9.81), torque=None):
        """A Dynamics handle for `robot`."""
        return Dynamics(self, robot, mass, com, inertia, gravity, torque)

    def torque_score_traj(self, robot, dynamics, delta_t, inter_step, traj, out=None, tau=True):
        """traj [B][N+1][2D] (or one [N+1][2D]) -> dict(torque_ratio [B], static_ratio [B], torque_time_scale [B], worst
        [B][3][2], invalid [B], tau [B][Md][D]) of the inter_step-up-sampled trajectories by inverse dynamics against the
        limits of `dynamics` (a Dynamics).  tau = False: the torques themselves are not fetched (tau: None)."""
        t, inter_step, delta_t, B, N = traj_args(traj, robot.dof, delta_t, inter_step)
        o = scoring.torque_outputs(B, scoring.checked_states(N, inter_step), robot.dof, out, tau)
        self._ck(self.lib.gpmp2mi_torque_score_traj(robot.ptr, dynamics.ptr, delta_t, inter_step, B, N, dptr(t),
                                                    *out_ptrs(stages.TORQUE, o)))
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
                                              *out_ptrs(stages.RETIME, o)))
        return o

    def retime_traj(self, robot, limits, delta_t, inter_step, traj, max_rate=1.0, rate_start=None, rate_end=None,
                    out=None):
        """traj [B][N+1][2D] (or one [N+1][2D]) -> dict(sdot, u, stamps [B][Md], duration [B], status [B], achieved
        [B][4], dense_retimed [B][Md][2D]): the fastest speed profile along the unchanged path under the rate limits of
        `limits` (a MotionLimits; None: max_rate alone).  rate_start / rate_end: a forced rate, None = free."""
        t, inter_step, delta_t, B, N = traj_args(traj, robot.dof, delta_t, inter_step)
        rates = scoring.retime_rates(max_rate, rate_start, rate_end)
        o = scoring.retime_outputs(B, scoring.checked_states(N, inter_step), robot.dof, out)
        lim = _limits_arg(limits, robot.dof)
        self._ck(self.lib.gpmp2mi_retime_traj(robot.ptr, lim, delta_t, inter_step, B, N, dptr(t), *rates,
                                              *out_ptrs(stages.RETIME, o)))
        return o

    # ---------------------------------------------------------------- re-timing under torque limits (include/gpmp2mi.h)
    def retime_path_affine(self, qd, qdd_left, qdd_right, cap, acc, cx_left, cx_right, cu, off, bound, h, max_rate=1.0,
                           rate_start=None, rate_end=None, out=None):
        """retime_path() with R affine rows |cx x + cu u + off| <= bound per state next to its own: cx_left, cx_right, cu,
        off [B][Md][R] (or one [Md][R]), bound [R] (inf: none; None or empty: R = 0) -> dict(sdot, u, stamps [B][Md],
        duration [B], status [B], achieved [B][6])."""
        q = np.ascontiguousarray(qd, dtype=np.float64)
        q = q[None] if q.ndim == 2 else q
        if q.ndim != 3 or q.shape[1] < 2:
            raise ValueError(f"qd: expected [B][Md][D] with Md >= 2, got {list(np.shape(qd))}")
        B, Md, D = q.shape
        ql, qr = (np.ascontiguousarray(x, dtype=np.float64).reshape(q.shape) for x in (qdd_left, qdd_right))
        c = np.ascontiguousarray(cap, dtype=np.float64).reshape(B, Md)
        a = None if acc is None else scoring.motion_limits(D, acc=acc)[3]
        R, cxl, cxr, ccu, cof, b = scoring.affine_rows(B, Md, cx_left, cx_right, cu, off, bound)
        if not (np.isfinite(float(h)) and float(h) > 0):
            raise ValueError("h must be finite and > 0")
        rates = scoring.retime_rates(max_rate, rate_start, rate_end)
        o = scoring.retime_affine_outputs(B, Md, out)
        rows = [dptr(x) if R else None for x in (cxl, cxr, ccu, cof, b)]
        self._ck(self.lib.gpmp2mi_retime_path_affine(B, Md, D, dptr(q), dptr(ql), dptr(qr), dptr(c), dptr(a), R, *rows,
                                                     float(h), *rates, *out_ptrs(stages.RETIME_AFFINE, o)))
        return o

    def retime_dynamic_traj(self, robot, dynamics, limits, delta_t, inter_step, traj, max_rate=1.0, rate_start=None,
                            rate_end=None, out=None, tau=True, coef=True):
        """traj [B][N+1][2D] (or one [N+1][2D]) -> dict(sdot, u, stamps [B][Md], duration [B], status [B], achieved
        [B][6], dense_retimed [B][Md][2D], tau_retimed [B][Md][D], coef [B][Md][4][D]): the fastest speed profile along
        the unchanged path under the torque limits of `dynamics` (a Dynamics) and the rate limits of `limits` (a
        MotionLimits; None: max_rate alone), with the torques the re-timed row asks for and the coefficients p, m_left,
        m_right, tau_g of tau = p u + m x + tau_g.  tau / coef = False: not fetched (None)."""
        t, inter_step, delta_t, B, N = traj_args(traj, robot.dof, delta_t, inter_step)
        rates = scoring.retime_rates(max_rate, rate_start, rate_end)
        o = scoring.retime_dynamic_outputs(B, scoring.checked_states(N, inter_step), robot.dof, out, tau, coef)
        lim = _limits_arg(limits, robot.dof)
        self._ck(self.lib.gpmp2mi_retime_dynamic_traj(robot.ptr, dynamics.ptr, lim, delta_t, inter_step, B, N, dptr(t),
                                                      *rates, *out_ptrs(stages.RETIME_DYNAMIC, o)))
        return o

    # ---------------------------------------------------------------- moving obstacles (include/gpmp2mi.h)
    def moving_score_traj(self, robot, radius, centers, epsilon, delta_t, inter_step, traj, out=None):
        """traj [B][N+1][2D] (or one [N+1][2D]) against the spheres radius [K], centers [K][N+1][3] -> dict(
        moving_support_cost [B], moving_dense_cost [B], min_moving_clearance [B], worst [B][3] = (checked state, robot
        sphere, moving sphere), invalid [B]) of the inter_step-up-sampled trajectories."""
        t, inter_step, delta_t, B, N = traj_args(traj, robot.dof, delta_t, inter_step)
        K, r, c = scoring.moving_set(radius, centers, N + 1)
        o = stages.outputs(stages.MOVING, B, out=out)
        self._ck(self.lib.gpmp2mi_moving_score_traj(robot.ptr, K, dptr(r), dptr(c), float(epsilon), delta_t,
                                                    inter_step, B, N, dptr(t), *out_ptrs(stages.MOVING, o)))
        return o

    # ---------------------------------------------------------------- carried object (include/gpmp2mi.h)
    def carried_score_traj(self, robot, sdf, link, radius, centers, delta_t, inter_step, traj, out=None):
        """traj [B][N+1][2D] (or one [N+1][2D]) with the spheres radius [A], centers [A][3] attached to `link`, against
        the field -> dict(carried_support_cost [B], carried_dense_cost [B], min_carried_clearance [B], worst [B][2] =
        (checked state, carried sphere), out_of_range [B]) of the inter_step-up-sampled trajectories."""
        t, inter_step, delta_t, B, N = traj_args(traj, robot.dof, delta_t, inter_step)
        A, r, c = scoring.carried_set(radius, centers)
        o = stages.outputs(stages.CARRIED, B, out=out)
        self._ck(self.lib.gpmp2mi_carried_score_traj(robot.ptr, sdf.ptr, int(link), A, dptr(r), dptr(c), delta_t,
                                                     inter_step, B, N, dptr(t), *out_ptrs(stages.CARRIED, o)))
        return o

    def carried_score_traj_dev(self, robot, sdf, link, A, radius, centers, delta_t, inter_step, B, N, traj,
                               carried_support_cost=None, carried_dense_cost=None, min_carried_clearance=None,
                               worst=None, out_of_range=None, stream=None):
        """The same on device buffers (torch tensors or raw pointers; any output may be None); no host synchronisation."""
        A, B, N = int(A), int(B), int(N)
        lead = [_dev_arg("radius", radius, (A,)), _dev_arg("centers", centers, (A, 3))]
        t = _dev_arg("traj", traj, (B, N + 1, 2 * robot.dof))
        args = dev_args(stages.CARRIED, B, None, None, locals())
        self._ck(self.lib.gpmp2mi_carried_score_traj_dev(robot.ptr, sdf.ptr, int(link), A, *lead, float(delta_t),
                                                         int(inter_step), B, N, t, *args, C.c_void_p(stream or 0)))

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
        t, inter_step, delta_t, B, N = traj_args(traj, robot.dof, delta_t, inter_step)
        d, s = scoring.path_arrays(des, sigma, N + 1)
        o = stages.outputs(stages.PATH, B, out=out)
        self._ck(self.lib.gpmp2mi_path_score_traj(robot.ptr, int(mode), int(link), dptr(d), dptr(s), delta_t,
                                                  inter_step, B, N, dptr(t), *out_ptrs(stages.PATH, o)))
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
