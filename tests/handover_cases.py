"""The plans of tests/test_gpu_handover_stores.py and what is recorded of each (shared with
scripts/record_handover_golden.py, which writes the fixture on the GPU at the commit whose results are to be kept).

Shapes: the smallest at which the order and flavour of the stores between the kernels of a pass can matter --
  N = 1, 2   no fused level 2: k_assemble returns before its group barrier
  N = 3      level 2 is the top level
  N = 4, 5   the last group of four is partly empty
  N = 8, 11  first level-4 and first level-8 task of the step kernels
on a planar two-link arm with three trajectories, of which the last starts at its optimum (error 0: it leaves in pass
0 and its hand-over tiles are never written), for Gauss-Newton, LM and Dogleg; one Pose2 plan (BASELINE config 5 cut to
N = 8: k_assemble<D, true>) and one 7-joint plan at N = 11.
"""
from __future__ import annotations

import ctypes as C
import hashlib

import numpy as np

import gpmp2_amd as g
from gpmp2_amd import datasets, problems
from gpmp2_amd.settings import TrajOptimizerSetting
from gpmp2_amd.trajutils import initArmTrajStraightLine

B = 3
PLANAR_N = [1, 2, 3, 4, 5, 8, 11]
OPTS = ["GN", "LM", "DOGLEG"]
RAW = {"tiles": 0, "fac": 1, "pend": 2, "coup": 3}      # gpmp2mi_plan_debug_read
RESULT_KEYS = ("traj", "iters", "status", "final_error")
ALREADY_OPTIMAL_ROW = B - 1


def planar2(N, opt):
    D = 2
    arm = g.Arm(D, [0.9 / D] * D, [0.0] * D, [0.0] * D)
    model = g.ArmModel(arm, [g.BodySphere(l, 0.05, (-0.45 / D, 0, 0)) for l in range(D)])
    d = datasets.generate2Ddataset("TwoObstaclesDataset")
    fld = datasets.signedDistanceField2D(d.map, d.cell_size)
    st = TrajOptimizerSetting(D)
    st.set_total_step(N); st.set_total_time(3.0); st.set_obs_check_inter(2); st.set_cost_sigma(0.1); st.set_epsilon(0.2)
    st.set_conf_prior_model(1e-3); st.set_vel_prior_model(1e-3); st.set_Qc_model(np.eye(D)); st.set_max_iter(12)
    {"GN": st.setGaussNewton, "LM": st.setLM, "DOGLEG": st.setDogleg}[opt]()
    rng = np.random.default_rng(42)
    start = np.zeros((B, D))
    end = np.linspace(0.3, 0.9, D)[None] + 0.2 * rng.normal(size=(B, D))
    end[ALREADY_OPTIMAL_ROW] = 0.0      # at rest in free space from start to end: every factor's error is exactly 0
    init = np.stack([initArmTrajStraightLine(start[b], end[b], N) for b in range(B)])
    z = np.zeros((B, D))
    return problems.Problem(f"planar arm N={N} {opt}", model, [d.origin_x, d.origin_y], d.cell_size, fld, st, start, z,
                            end, z.copy(), init)


def pose2_n8():
    p = problems.mobile_arm_config5()
    N, D = 8, 5
    p.setting.set_total_step(N)
    p.setting.set_max_iter(12)
    start, end = p.start_conf[0], p.end_conf[0]
    dt = 5.0 / N
    avg_vel = np.concatenate([end[:3] - start[:3], end[3:] / N]) / dt
    init = np.zeros((1, N + 1, 2 * D))
    for i in range(N + 1):
        init[0, i, :D] = start * (N - i) / N + end * i / N
        init[0, i, D:] = avg_vel
    p.init = init
    return p


def wam_n11():
    return problems.wam_restarts(B=B, total_step=11, obs_check_inter=2, opt="GN", sdf="40", max_iter=12)


def cases():
    out = {f"planar2_N{N}_{opt}": (lambda N=N, opt=opt: planar2(N, opt)) for opt in OPTS for N in PLANAR_N}
    out["pose2_N8_DOGLEG"] = pose2_n8
    out["wam_N11_GN"] = wam_n11
    return out


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(engine, make):
    """-> {"traj", "iters", "status", "final_error"} of the whole plan and, under "raw", the SHA-256 of the bytes of
    tiles / fac / pend / coup as the plan's last pass left them (the arena starts zeroed, so every byte is defined)"""
    p = make()
    nb, N = p.init.shape[0], p.init.shape[1] - 1
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pl = engine.plan(r, s, p.setting, nb)
    try:
        pl.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
        pl.optimize()
        res = pl.result()
        out = {k: np.array(res[k]) for k in RESULT_KEYS}
        groups = (N + 1) // 4 + 1                    # cr_schedule.h crr_groups(N, 4): tree indices 0 .. N + 1 in fours
        count = {"tiles": nb * (N + 1) * 256, "fac": nb * (N + 1) * 768, "pend": nb * groups * 256,
                 "coup": nb * groups * 256}
        raw = {}
        for name, which in RAW.items():
            a = np.zeros(count[name])
            engine._ck(engine.lib.gpmp2mi_plan_debug_read(pl.h.ptr, which, a.ctypes.data_as(C.POINTER(C.c_double)),
                                                          C.c_long(a.size)))
            raw[name] = _digest(a)
        out["raw"] = raw
    finally:
        pl.close()
    return out
