"""Plan and MultiPlan: the resident batch of trajectory problems of include/gpmp2mi.h ("the planner", "a queue of
problems", "one batch sharded across several GPUs") with the check stages, selections and posterior calls on its result.
The selections share one host body and one `_dev` body (selection_host, selection_dev)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi, scoring, stages
from ._capi import dptr, f64, iptr
from .marshalling import (_dev_arg, _Handle, _kappa_arg, _limits_arg, _sampled_dev_args, _sampled_ptrs, _score_args,
                          dev_args, multi_plan_args, out_ptrs, queue_inputs, sampled_args, sampled_outputs, seed_inputs)


def threshold_args(required_clearance, require_in_range, *self_check):
    """The leading thresholds of a selection, in header order.  self_check: (pairs, required_self_clearance) for the
    selections whose rule has the self-collision conditions; pairs None (not asked) is a null table."""
    lead = [float(required_clearance), int(bool(require_in_range))]
    if self_check:
        pairs, required_self_clearance = self_check
        lead += [None if pairs is None else pairs.ptr, float(required_self_clearance)]
    return lead


def _selected(N, D, Md, scalar, row):
    """(name, shape, integer) of the outputs of a selection, in C argument order: best, n_eligible, the optional extra
    scalar and extra row ((name, shape per checked state)) of the chosen row, traj_best, dense_best."""
    rows = [] if row is None else [row] if isinstance(row[0], str) else list(row)      # one extra row, or several
    return ([("best", (1,), True), ("n_eligible", (1,), True)] + ([] if scalar is None else [(scalar, (1,), False)])
            + [(name, (Md,) + tuple(tail), False) for name, tail in rows]
            + [("traj_best", (N + 1, 2 * D), False), ("dense_best", (Md, 2 * D), False)])


def selection_host(pl, fn, inter_step, lead, scalar=None, row=None):
    """One selection of a plan's (or multi plan's) result with host outputs: calls the entry point named fn as
    fn(plan, inter_step, *lead, outputs) and returns dict(best, n_eligible, [scalar], [row], traj_best, dense_best),
    everything about the chosen row None when best < 0.  lead: the thresholds and handles between inter_step and the
    outputs, in header order."""
    Md = scoring.checked_states(pl.N, inter_step)
    o = {name: np.zeros(shape, dtype=np.int32 if integer else np.float64)
         for name, shape, integer in _selected(pl.N, pl.D, Md, scalar, row)}
    o["best"][0] = -1
    ptrs = [(iptr if x.dtype == np.int32 else dptr)(x) for x in o.values()]
    pl.eng._ck(getattr(pl.eng.lib, fn)(pl.h.ptr, inter_step, *lead, *ptrs))
    res = dict(best=int(o.pop("best")[0]), n_eligible=int(o.pop("n_eligible")[0]))
    for name, x in o.items():
        res[name] = None if res["best"] < 0 else float(x[0]) if name == scalar else x
    return res


def selection_dev(pl, fn, inter_step, lead, given, scalar=None, row=None):
    """The same with device outputs: given[name] is the caller's buffer for each output and given["stream"] the stream
    (a method passes its locals()), checked before the library is looked at.  One enqueue, no host synchronisation."""
    Md = scoring.checked_states(pl.N, inter_step)
    args = [_dev_arg(name, given[name], shape, integer) for name, shape, integer in _selected(pl.N, pl.D, Md, scalar, row)]
    pl.eng._ck(getattr(pl.eng.lib, fn)(pl.h.ptr, inter_step, *lead, *args, C.c_void_p(given["stream"] or 0)))


def solved_rows(pl, M):
    """Fresh host arrays for the outputs of a solve of M problems (the result() dict) and their pointers, both in C
    argument order."""
    o = dict(traj=np.zeros((M, pl.N + 1, 2 * pl.D)), iters=np.zeros(M, dtype=np.int32), final_error=np.zeros(M),
             status=np.zeros(M, dtype=np.int32), error_trace=np.zeros((M, pl.setting.max_iter + 1)))
    return o, [(iptr if x.dtype == np.int32 else dptr)(x) for x in o.values()]


def queue_host(pl, fn, start_conf, start_vel, end_conf, end_vel, init):
    """M problems through a plan or a multi plan (fn: the entry point's name): the result() dict with M rows."""
    M, (sc, sv, ec, ev), t = queue_inputs(pl.D, pl.N, start_conf, start_vel, end_conf, end_vel, init)
    o, ptrs = solved_rows(pl, M)
    pl.eng._ck(getattr(pl.eng.lib, fn)(pl.h.ptr, M, dptr(sc), dptr(sv), dptr(ec), dptr(ev), dptr(t), *ptrs))
    return o


def queue_seeded_host(pl, fn, seed, start_conf, start_vel, end_conf, end_vel, mean, first, scale, keep_first, want_init):
    """The same on M restarts made on the device; `init` joins the dict when want_init."""
    D, N = pl.D, pl.N
    rows = [f64(x).reshape(-1, D) for x in (start_conf, start_vel, end_conf, end_vel)]
    M, sc, ec, mu = seed_inputs(D, N, rows[0], rows[2], mean)
    if any(x.shape[0] != M for x in rows):
        raise ValueError(f"queue inputs disagree on the number of problems: {[x.shape[0] for x in rows]}")
    o, ptrs = solved_rows(pl, M)
    init = np.zeros((M, N + 1, 2 * D)) if want_init else None
    pl.eng._ck(getattr(pl.eng.lib, fn)(pl.h.ptr, M, int(seed), int(first), float(scale), int(bool(keep_first)), dptr(sc),
                                       dptr(rows[1]), dptr(ec), dptr(rows[3]), dptr(mu), *ptrs, dptr(init)))
    if want_init:
        o["init"] = init
    return o


class Plan:
    """gpmp2mi_plan: B trajectory problems resident on the GPU.  forms (tests, probes): a dict of the kernel forms to force
    on the plan, e.g. {"lin_split": 2} (gpmp2mi_debug_forms, include/gpmp2mi_debug.h); None: the plan's own choice."""

    def __init__(self, eng, robot, sdf, setting, B: int, forms=None):
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
        o, ptrs = solved_rows(self, self.B)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_get_result(self.h.ptr, *ptrs))
        return o

    def result_counts(self):
        B = self.B
        iters, status, ferr = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), np.zeros(B)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_get_result(self.h.ptr, None, iptr(iters), dptr(ferr), iptr(status), None))
        return iters, status, ferr

    # ---- a queue of problems through the plan's B slots (gpmp2mi_plan_optimize_queue, include/gpmp2mi.h)
    def optimize_queue(self, start_conf, start_vel, end_conf, end_vel, init):
        """M problems ([M][D] x 4, [M][N+1][2D], host arrays): the result() dict with M rows, row j = problem j."""
        return queue_host(self, "gpmp2mi_plan_optimize_queue", start_conf, start_vel, end_conf, end_vel, init)

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
            if x is None and len(args) < 5:
                raise ValueError(f"{name} is required")
            args.append(_dev_arg(name, x, shape, name in ints))
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
        return queue_seeded_host(self, "gpmp2mi_plan_optimize_queue_seeded", seed, start_conf, start_vel, end_conf, end_vel,
                                 mean, first, scale, keep_first, want_init)

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
        o = stages.outputs(stages.SCORE, self.B, out=out)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_score(self.h.ptr, inter_step, *out_ptrs(stages.SCORE, o)))
        return o

    def score_dev(self, inter_step, support_cost=None, dense_cost=None, min_clearance=None, worst=None,
                  out_of_range=None, stream=None):
        """The same into device buffers (torch tensors or raw pointers, any may be None); no host synchronisation."""
        args = dev_args(stages.SCORE, self.B, None, None, locals())
        self.eng._ck(self.eng.lib.gpmp2mi_plan_score_dev(self.h.ptr, _score_args(inter_step), *args,
                                                         C.c_void_p(stream or 0)))

    def select(self, inter_step, required_clearance=0.0, require_in_range=False):
        """Score, apply the rule to the plan's final_error / status, fetch the chosen row: dict(best, n_eligible,
        traj_best [N+1][2D], dense_best [Md][2D]); best = -1: the two trajectories are None."""
        inter_step = _score_args(inter_step)
        lead = threshold_args(required_clearance, require_in_range)
        return selection_host(self, "gpmp2mi_plan_select", inter_step, lead)

    def select_dev(self, inter_step, required_clearance=0.0, require_in_range=False, best=None, n_eligible=None,
                   traj_best=None, dense_best=None, stream=None):
        """The same with device outputs: best / n_eligible int32 [1], traj_best [N+1][2D], dense_best [Md][2D] (torch
        tensors or raw pointers, any may be None).  One enqueue on `stream`, no host synchronisation."""
        inter_step = _score_args(inter_step)
        lead = threshold_args(required_clearance, require_in_range)
        selection_dev(self, "gpmp2mi_plan_select_dev", inter_step, lead, locals())

    # ---- the same against the robot itself (include/gpmp2mi.h "self-collision check")
    def self_score(self, pairs, inter_step, out=None):
        """dict(self_support_cost, self_dense_cost, min_self_clearance, worst, invalid) of the plan's result, B rows."""
        inter_step = _score_args(inter_step)
        o = stages.outputs(stages.SELF, self.B, out=out)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_self_score(self.h.ptr, pairs.ptr, inter_step, *out_ptrs(stages.SELF, o)))
        return o

    def self_score_dev(self, pairs, inter_step, self_support_cost=None, self_dense_cost=None, min_self_clearance=None,
                       worst=None, invalid=None, stream=None):
        """The same into device buffers (torch tensors or raw pointers, any may be None); no host synchronisation."""
        args = dev_args(stages.SELF, self.B, None, None, locals())
        self.eng._ck(self.eng.lib.gpmp2mi_plan_self_score_dev(self.h.ptr, pairs.ptr, _score_args(inter_step), *args,
                                                              C.c_void_p(stream or 0)))

    def select_checked(self, inter_step, pairs, required_clearance=0.0, require_in_range=False,
                       required_self_clearance=0.0):
        """select() with the rule that also asks for required_self_clearance against the pairs of `pairs` and no invalid
        pair: dict(best, n_eligible, traj_best, dense_best); best = -1: the two trajectories are None."""
        inter_step = _score_args(inter_step)
        lead = threshold_args(required_clearance, require_in_range, pairs, required_self_clearance)
        return selection_host(self, "gpmp2mi_plan_select_checked", inter_step, lead)

    def select_checked_dev(self, inter_step, pairs, required_clearance=0.0, require_in_range=False,
                           required_self_clearance=0.0, best=None, n_eligible=None, traj_best=None, dense_best=None,
                           stream=None):
        """The same with device outputs, as select_dev.  One enqueue on `stream`, no host synchronisation."""
        inter_step = _score_args(inter_step)
        lead = threshold_args(required_clearance, require_in_range, pairs, required_self_clearance)
        selection_dev(self, "gpmp2mi_plan_select_checked_dev", inter_step, lead, locals())

    # ---- can the robot execute it (include/gpmp2mi.h "motion limits")
    def motion_score(self, limits, inter_step, out=None):
        """dict(pos_margin, vel_ratio, acc_ratio, point_speed, time_scale, worst, invalid) of the plan's result, B rows."""
        inter_step = _score_args(inter_step)
        o = stages.outputs(stages.MOTION, self.B, out=out)
        lim = _limits_arg(limits, self.D)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_motion_score(self.h.ptr, lim, inter_step, *out_ptrs(stages.MOTION, o)))
        return o

    def motion_score_dev(self, limits, inter_step, pos_margin=None, vel_ratio=None, acc_ratio=None, point_speed=None,
                         time_scale=None, worst=None, invalid=None, stream=None):
        """The same into device buffers (torch tensors or raw pointers, any may be None); no host synchronisation."""
        args = dev_args(stages.MOTION, self.B, None, None, locals())
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
        lead = threshold_args(required_clearance, require_in_range, pairs, required_self_clearance)
        lead += [_limits_arg(limits, self.D), rpm, mts]
        return selection_host(self, "gpmp2mi_plan_select_feasible", inter_step, lead, "time_scale_best")

    def select_feasible_dev(self, inter_step, limits, required_pos_margin=0.0, max_time_scale=1.0, required_clearance=0.0,
                            require_in_range=False, pairs=None, required_self_clearance=0.0, best=None, n_eligible=None,
                            time_scale_best=None, traj_best=None, dense_best=None, stream=None):
        """The same with device outputs, as select_dev, plus time_scale_best float64 [1].  One enqueue on `stream`, no
        host synchronisation once the plan's workspaces hold the shape."""
        inter_step = _score_args(inter_step)
        rpm, mts = scoring.feasible_thresholds(required_pos_margin, max_time_scale)
        lead = threshold_args(required_clearance, require_in_range, pairs, required_self_clearance)
        lead += [_limits_arg(limits, self.D), rpm, mts]
        selection_dev(self, "gpmp2mi_plan_select_feasible_dev", inter_step, lead, locals(), "time_scale_best")

    # ---- can the drives produce it (include/gpmp2mi.h "torque limits")
    def torque_score(self, dynamics, inter_step, out=None, tau=True):
        """dict(torque_ratio, static_ratio, torque_time_scale, worst, invalid, tau) of the plan's result, B rows."""
        inter_step = _score_args(inter_step)
        o = scoring.torque_outputs(self.B, scoring.checked_states(self.N, inter_step), self.D, out, tau)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_torque_score(self.h.ptr, dynamics.ptr, inter_step,
                                                            *out_ptrs(stages.TORQUE, o)))
        return o

    def torque_score_dev(self, dynamics, inter_step, torque_ratio=None, static_ratio=None, torque_time_scale=None,
                         worst=None, invalid=None, tau=None, stream=None):
        """The same into device buffers (torch tensors or raw pointers, any may be None); no host synchronisation."""
        inter_step = _score_args(inter_step)
        args = dev_args(stages.TORQUE, self.B, scoring.checked_states(self.N, inter_step), self.D, locals())
        self.eng._ck(self.eng.lib.gpmp2mi_plan_torque_score_dev(self.h.ptr, dynamics.ptr, inter_step, *args,
                                                                C.c_void_p(stream or 0)))

    def select_dynamic(self, inter_step, limits, dynamics, required_pos_margin=0.0, max_time_scale=1.0,
                       required_clearance=0.0, require_in_range=False, pairs=None, required_self_clearance=0.0):
        """select_feasible() with max(time_scale, torque_time_scale) <= max_time_scale in place of its time-scale test
        and no non-finite torque: dict(best, n_eligible, time_scale_best, tau_best, traj_best, dense_best); best = -1:
        the last four are None.  time_scale_best is that maximum; tau_best [Md][D] are the torques at planned timing."""
        inter_step = _score_args(inter_step)
        rpm, mts = scoring.feasible_thresholds(required_pos_margin, max_time_scale)
        lead = threshold_args(required_clearance, require_in_range, pairs, required_self_clearance)
        lead += [_limits_arg(limits, self.D), rpm, mts, dynamics.ptr]
        return selection_host(self, "gpmp2mi_plan_select_dynamic", inter_step, lead, "time_scale_best",
                              ("tau_best", (self.D,)))

    def select_dynamic_dev(self, inter_step, limits, dynamics, required_pos_margin=0.0, max_time_scale=1.0,
                           required_clearance=0.0, require_in_range=False, pairs=None, required_self_clearance=0.0,
                           best=None, n_eligible=None, time_scale_best=None, tau_best=None, traj_best=None,
                           dense_best=None, stream=None):
        """The same with device outputs, as select_feasible_dev, plus tau_best float64 [Md][D].  One enqueue on `stream`,
        no host synchronisation once the plan's workspaces hold the shape."""
        inter_step = _score_args(inter_step)
        rpm, mts = scoring.feasible_thresholds(required_pos_margin, max_time_scale)
        lead = threshold_args(required_clearance, require_in_range, pairs, required_self_clearance)
        lead += [_limits_arg(limits, self.D), rpm, mts, dynamics.ptr]
        selection_dev(self, "gpmp2mi_plan_select_dynamic_dev", inter_step, lead, locals(), "time_scale_best",
                      ("tau_best", (self.D,)))

    # ---- how fast can the robot run it (include/gpmp2mi.h "re-timing")
    def retime(self, limits, inter_step, max_rate=1.0, rate_start=None, rate_end=None, out=None):
        """dict(sdot, u, stamps, duration, status, achieved, dense_retimed) of the plan's result, B rows."""
        inter_step = _score_args(inter_step)
        rates = scoring.retime_rates(max_rate, rate_start, rate_end)
        o = scoring.retime_outputs(self.B, scoring.checked_states(self.N, inter_step), self.D, out)
        lim = _limits_arg(limits, self.D)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_retime(self.h.ptr, lim, inter_step, *rates, *out_ptrs(stages.RETIME, o)))
        return o

    def retime_dev(self, limits, inter_step, max_rate=1.0, rate_start=None, rate_end=None, sdot=None, u=None,
                   stamps=None, duration=None, status=None, achieved=None, dense_retimed=None, stream=None):
        """The same into device buffers (torch tensors or raw pointers, any may be None); no host synchronisation."""
        inter_step = _score_args(inter_step)
        rates = scoring.retime_rates(max_rate, rate_start, rate_end)
        args = dev_args(stages.RETIME, self.B, scoring.checked_states(self.N, inter_step), self.D, locals())
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
        lead = threshold_args(required_clearance, require_in_range, pairs, required_self_clearance)
        lead += [_limits_arg(limits, self.D), rpm, *rates, md]
        return selection_host(self, "gpmp2mi_plan_select_retimed", inter_step, lead, "duration_best",
                              ("stamps_best", ()))

    def select_retimed_dev(self, inter_step, limits, required_pos_margin=0.0, max_duration=np.inf, max_rate=1.0,
                           rate_start=None, rate_end=None, required_clearance=0.0, require_in_range=False, pairs=None,
                           required_self_clearance=0.0, best=None, n_eligible=None, duration_best=None,
                           stamps_best=None, traj_best=None, dense_best=None, stream=None):
        """The same with device outputs, as select_feasible_dev, plus duration_best float64 [1] and stamps_best [Md].
        One enqueue on `stream`, no host synchronisation once the plan's workspaces hold the shape."""
        inter_step = _score_args(inter_step)
        rpm, md = scoring.retimed_thresholds(required_pos_margin, max_duration)
        rates = scoring.retime_rates(max_rate, rate_start, rate_end)
        lead = threshold_args(required_clearance, require_in_range, pairs, required_self_clearance)
        lead += [_limits_arg(limits, self.D), rpm, *rates, md]
        selection_dev(self, "gpmp2mi_plan_select_retimed_dev", inter_step, lead, locals(), "duration_best",
                      ("stamps_best", ()))

    # ---- how fast can the drives run it (include/gpmp2mi.h "re-timing under torque limits")
    def retime_dynamic(self, dynamics, limits, inter_step, max_rate=1.0, rate_start=None, rate_end=None, out=None,
                       tau=True, coef=True):
        """dict(sdot, u, stamps, duration, status, achieved [B][6], dense_retimed, tau_retimed, coef) of the plan's
        result, B rows: retime() with the torque limits of `dynamics` in the profile."""
        inter_step = _score_args(inter_step)
        rates = scoring.retime_rates(max_rate, rate_start, rate_end)
        o = scoring.retime_dynamic_outputs(self.B, scoring.checked_states(self.N, inter_step), self.D, out, tau, coef)
        lim = _limits_arg(limits, self.D)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_retime_dynamic(self.h.ptr, dynamics.ptr, lim, inter_step, *rates,
                                                              *out_ptrs(stages.RETIME_DYNAMIC, o)))
        return o

    def retime_dynamic_dev(self, dynamics, limits, inter_step, max_rate=1.0, rate_start=None, rate_end=None, sdot=None,
                           u=None, stamps=None, duration=None, status=None, achieved=None, dense_retimed=None,
                           tau_retimed=None, coef=None, stream=None):
        """The same into device buffers (torch tensors or raw pointers, any may be None); no host synchronisation."""
        inter_step = _score_args(inter_step)
        rates = scoring.retime_rates(max_rate, rate_start, rate_end)
        args = dev_args(stages.RETIME_DYNAMIC, self.B, scoring.checked_states(self.N, inter_step), self.D, locals())
        lim = _limits_arg(limits, self.D)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_retime_dynamic_dev(self.h.ptr, dynamics.ptr, lim, inter_step, *rates, *args,
                                                                  C.c_void_p(stream or 0)))

    def select_retimed_dynamic(self, inter_step, limits, dynamics, required_pos_margin=0.0, max_duration=np.inf,
                               max_rate=1.0, rate_start=None, rate_end=None, required_clearance=0.0,
                               require_in_range=False, pairs=None, required_self_clearance=0.0):
        """select_retimed() on the profile under the torque limits of `dynamics`, and no coefficient that is not finite:
        dict(best, n_eligible, duration_best, stamps_best, tau_best, traj_best, dense_best); best = -1: the last five are
        None.  tau_best [Md][D] are the torques the re-timed row asks for."""
        inter_step = _score_args(inter_step)
        rpm, md = scoring.retimed_thresholds(required_pos_margin, max_duration)
        rates = scoring.retime_rates(max_rate, rate_start, rate_end)
        lead = threshold_args(required_clearance, require_in_range, pairs, required_self_clearance)
        lead += [_limits_arg(limits, self.D), rpm, *rates, md, dynamics.ptr]
        return selection_host(self, "gpmp2mi_plan_select_retimed_dynamic", inter_step, lead, "duration_best",
                              (("stamps_best", ()), ("tau_best", (self.D,))))

    def select_retimed_dynamic_dev(self, inter_step, limits, dynamics, required_pos_margin=0.0, max_duration=np.inf,
                                   max_rate=1.0, rate_start=None, rate_end=None, required_clearance=0.0,
                                   require_in_range=False, pairs=None, required_self_clearance=0.0, best=None,
                                   n_eligible=None, duration_best=None, stamps_best=None, tau_best=None, traj_best=None,
                                   dense_best=None, stream=None):
        """The same with device outputs, as select_retimed_dev, plus tau_best float64 [Md][D].  One enqueue on `stream`,
        no host synchronisation once the plan's workspaces hold the shape."""
        inter_step = _score_args(inter_step)
        rpm, md = scoring.retimed_thresholds(required_pos_margin, max_duration)
        rates = scoring.retime_rates(max_rate, rate_start, rate_end)
        lead = threshold_args(required_clearance, require_in_range, pairs, required_self_clearance)
        lead += [_limits_arg(limits, self.D), rpm, *rates, md, dynamics.ptr]
        selection_dev(self, "gpmp2mi_plan_select_retimed_dynamic_dev", inter_step, lead, locals(), "duration_best",
                      (("stamps_best", ()), ("tau_best", (self.D,))))

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
        o = stages.outputs(stages.MOVING, self.B, out=out)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_moving_score(self.h.ptr, inter_step, *out_ptrs(stages.MOVING, o)))
        return o

    def moving_score_dev(self, inter_step, moving_support_cost=None, moving_dense_cost=None, min_moving_clearance=None,
                         worst=None, invalid=None, stream=None):
        """The same into device buffers (torch tensors or raw pointers, any may be None); no host synchronisation."""
        args = dev_args(stages.MOVING, self.B, None, None, locals())
        self.eng._ck(self.eng.lib.gpmp2mi_plan_moving_score_dev(self.h.ptr, _score_args(inter_step), *args,
                                                                C.c_void_p(stream or 0)))

    def select_moving(self, inter_step, required_moving_clearance=0.0, required_clearance=0.0, require_in_range=False,
                      pairs=None, required_self_clearance=0.0):
        """select() (select_checked() when `pairs` is given) with the rule that also asks for no invalid pair and
        required_moving_clearance against the plan's sphere set: dict(best, n_eligible, traj_best, dense_best);
        best = -1: the two trajectories are None."""
        inter_step = _score_args(inter_step)
        lead = threshold_args(required_clearance, require_in_range, pairs, required_self_clearance)
        lead.append(float(required_moving_clearance))
        return selection_host(self, "gpmp2mi_plan_select_moving", inter_step, lead)

    def select_moving_dev(self, inter_step, required_moving_clearance=0.0, required_clearance=0.0, require_in_range=False,
                          pairs=None, required_self_clearance=0.0, best=None, n_eligible=None, traj_best=None,
                          dense_best=None, stream=None):
        """The same with device outputs, as select_dev.  One enqueue on `stream`, no host synchronisation once the
        plan's workspaces hold the shape."""
        inter_step = _score_args(inter_step)
        lead = threshold_args(required_clearance, require_in_range, pairs, required_self_clearance)
        lead.append(float(required_moving_clearance))
        selection_dev(self, "gpmp2mi_plan_select_moving_dev", inter_step, lead, locals())

    # ---- spheres rigidly attached to one link (include/gpmp2mi.h "carried object")
    def set_carried(self, link, radius, centers):
        """The plan's carried set: radius [A], centers [A][3] in the frame of `link`; None / empty clears it.  May be
        repeated between solves; the plan must have been created with room for A
        (TrajOptimizerSetting.set_carried_spheres)."""
        A, r, c = scoring.carried_set(radius, centers)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_set_carried(self.h.ptr, int(link), A, dptr(r), dptr(c)))

    def set_carried_dev(self, link, A, radius, centers, stream=None):
        """The same from device buffers (torch tensors or raw pointers); the copies are enqueued on `stream`."""
        A = int(A)
        args = [_dev_arg("radius", radius, (A,)), _dev_arg("centers", centers, (A, 3))]
        self.eng._ck(self.eng.lib.gpmp2mi_plan_set_carried_dev(self.h.ptr, int(link), A, *args, C.c_void_p(stream or 0)))

    def carried_count(self):
        """spheres of the set resident in the plan"""
        return int(self.eng.lib.gpmp2mi_plan_carried_count(self.h.ptr))

    def carried_score(self, inter_step, out=None):
        """dict(carried_support_cost, carried_dense_cost, min_carried_clearance, worst [B][2], out_of_range) of the
        plan's result with its resident carried set against the plan's field, B rows."""
        inter_step = _score_args(inter_step)
        o = stages.outputs(stages.CARRIED, self.B, out=out)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_carried_score(self.h.ptr, inter_step, *out_ptrs(stages.CARRIED, o)))
        return o

    def carried_score_dev(self, inter_step, carried_support_cost=None, carried_dense_cost=None,
                          min_carried_clearance=None, worst=None, out_of_range=None, stream=None):
        """The same into device buffers (torch tensors or raw pointers, any may be None); no host synchronisation."""
        args = dev_args(stages.CARRIED, self.B, None, None, locals())
        self.eng._ck(self.eng.lib.gpmp2mi_plan_carried_score_dev(self.h.ptr, _score_args(inter_step), *args,
                                                                 C.c_void_p(stream or 0)))

    def select_carried(self, inter_step, required_carried_clearance=0.0, required_clearance=0.0, require_in_range=False,
                       pairs=None, required_self_clearance=0.0):
        """select() (select_checked() when `pairs` is given) with the rule that also asks for
        required_carried_clearance of the plan's carried set and, with require_in_range, for no carried sphere out of
        the field: dict(best, n_eligible, traj_best, dense_best); best = -1: the two trajectories are None."""
        inter_step = _score_args(inter_step)
        lead = threshold_args(required_clearance, require_in_range, pairs, required_self_clearance)
        lead.append(float(required_carried_clearance))
        return selection_host(self, "gpmp2mi_plan_select_carried", inter_step, lead)

    def select_carried_dev(self, inter_step, required_carried_clearance=0.0, required_clearance=0.0,
                           require_in_range=False, pairs=None, required_self_clearance=0.0, best=None, n_eligible=None,
                           traj_best=None, dense_best=None, stream=None):
        """The same with device outputs, as select_dev.  One enqueue on `stream`, no host synchronisation once the
        plan's workspaces hold the shape."""
        inter_step = _score_args(inter_step)
        lead = threshold_args(required_clearance, require_in_range, pairs, required_self_clearance)
        lead.append(float(required_carried_clearance))
        selection_dev(self, "gpmp2mi_plan_select_carried_dev", inter_step, lead, locals())

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
        o = stages.outputs(stages.PATH, self.B, out=out)
        self.eng._ck(self.eng.lib.gpmp2mi_plan_path_score(self.h.ptr, inter_step, *out_ptrs(stages.PATH, o)))
        return o

    def path_score_dev(self, inter_step, max_pos_dev=None, max_rot_dev=None, worst=None, support_cost=None,
                       dense_cost=None, invalid=None, stream=None):
        """The same into device buffers (torch tensors or raw pointers, any may be None); no host synchronisation."""
        args = dev_args(stages.PATH, self.B, None, None, locals())
        self.eng._ck(self.eng.lib.gpmp2mi_plan_path_score_dev(self.h.ptr, _score_args(inter_step), *args,
                                                              C.c_void_p(stream or 0)))

    def select_path(self, inter_step, max_pos_dev_allowed=np.inf, max_rot_dev_allowed=np.inf, required_clearance=0.0,
                    require_in_range=False):
        """select() with the rule that also asks for no invalid checked state and deviations from the plan's path
        within the two allowances: dict(best, n_eligible, traj_best, dense_best); best = -1: the two trajectories
        are None."""
        inter_step = _score_args(inter_step)
        lead = threshold_args(required_clearance, require_in_range) + [float(max_pos_dev_allowed), float(max_rot_dev_allowed)]
        return selection_host(self, "gpmp2mi_plan_select_path", inter_step, lead)

    def select_path_dev(self, inter_step, max_pos_dev_allowed=np.inf, max_rot_dev_allowed=np.inf, required_clearance=0.0,
                        require_in_range=False, best=None, n_eligible=None, traj_best=None, dense_best=None, stream=None):
        """The same with device outputs, as select_dev.  One enqueue on `stream`, no host synchronisation once the
        plan's workspaces hold the shape."""
        inter_step = _score_args(inter_step)
        lead = threshold_args(required_clearance, require_in_range) + [float(max_pos_dev_allowed), float(max_rot_dev_allowed)]
        selection_dev(self, "gpmp2mi_plan_select_path_dev", inter_step, lead, locals())

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
            self.h.ptr, inter_step, *threshold_args(required_clearance, require_in_range, pairs, required_self_clearance),
            metric, dptr(w), radius, max_alt, C.byref(nm), C.byref(ne), iptr(alt), iptr(size), dptr(err), iptr(mode), dptr(ta), dptr(da)))
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
            self.h.ptr, inter_step, *threshold_args(required_clearance, require_in_range, pairs, required_self_clearance),
            metric, dptr(w), radius, max_alt, *args, C.c_void_p(stream or 0)))

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

    def __init__(self, eng, robot, sdf, setting, B, devices, forms=None, replicate_all=False):
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
        o, ptrs = solved_rows(self, self.B)
        self.eng._ck(self.eng.lib.gpmp2mi_multi_plan_get_result(self.h.ptr, *ptrs))
        return o

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
        return queue_host(self, "gpmp2mi_multi_plan_optimize_queue", start_conf, start_vel, end_conf, end_vel, init)

    def optimize_queue_seeded(self, seed, start_conf, start_vel, end_conf, end_vel, mean=None, first=0, scale=1.0,
                              keep_first=False, want_init=False):
        """Plan.optimize_queue_seeded split over the shards: the same rows as one plan returns."""
        return queue_seeded_host(self, "gpmp2mi_multi_plan_optimize_queue_seeded", seed, start_conf, start_vel, end_conf,
                                 end_vel, mean, first, scale, keep_first, want_init)

    def score(self, inter_step, out=None):
        """Plan.score over all shards, rows in batch order."""
        inter_step = _score_args(inter_step)
        o = stages.outputs(stages.SCORE, self.B, out=out)
        self.eng._ck(self.eng.lib.gpmp2mi_multi_plan_score(self.h.ptr, inter_step, *out_ptrs(stages.SCORE, o)))
        return o

    def select(self, inter_step, required_clearance=0.0, require_in_range=False):
        """Plan.select over all shards: `best` is a batch row."""
        inter_step = _score_args(inter_step)
        lead = threshold_args(required_clearance, require_in_range)
        return selection_host(self, "gpmp2mi_multi_plan_select", inter_step, lead)

    def queue_stats(self, shard):
        """of the last queue run, shard `shard`: passes, slot_passes, busy_slot_passes (zeros if it had no problems)."""
        st = _capi.QueueStats()
        self.eng._ck(self.eng.lib.gpmp2mi_multi_plan_queue_stats(self.h.ptr, int(shard), C.byref(st)))
        return dict(passes=st.passes, slot_passes=st.slot_passes, busy_slot_passes=st.busy_slot_passes)
