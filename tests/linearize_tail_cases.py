"""The plans of tests/test_gpu_linearize_tail.py and what is recorded of each (shared with
scripts/record_linearize_tail_golden.py, which writes the fixture on the GPU at the commit whose results are to be kept).

The four-wavefront linearization (k_linearize_arm) sums two partial records per evaluation point, stores the chunk's 64
records in 16-byte pieces and evaluates the GP prior of its support states.  Shapes: the smallest at which who stores
which piece, and when, can matter --
  planar arms of 1, 2, 3, 4 joints      records of 3, 6, 10, 15 values: the last piece with and without the 0.0 pad
  the 7-joint WAM on the 40^3 field     the flagship's record (36 values, 18 pieces)
  P = 1 + N (I + 1) evaluation points, I = 2:
    N = 11  P = 34    one partial chunk
    N = 21  P = 64    exactly one full chunk
    N = 22  P = 67    a last chunk of 3 points
    N = 43  P = 130   three chunks, the fused finish across chunk borders
Every plan has three trajectories, of which the last starts at its optimum (error 0: it leaves in pass 0 and its
workgroups return at once); every link carries two spheres, so that the plan takes the four-wavefront form.  Gauss-Newton
and LM (the trial-step path of the kernel), and one fixed-iteration plan (gpmp2mi_plan_update, 2 iterations).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import gpmp2_amd as g
import handover_cases as hc
from gpmp2_amd import datasets, problems
from gpmp2_amd.settings import TrajOptimizerSetting
from gpmp2_amd.trajutils import initArmTrajStraightLine

B = hc.B
ALREADY_OPTIMAL_ROW = hc.ALREADY_OPTIMAL_ROW
RESULT_KEYS = hc.RESULT_KEYS
LIN_VALUE_KEYS = ("lin_g", "lin_err")          # kept as values
LIN_DIGEST_KEYS = ("Hdiag", "Hoff")            # kept as SHA-256
UPDATE_ITERATIONS = 2


def planar(D, N, opt):
    arm = g.Arm(D, [0.9 / D] * D, [0.0] * D, [0.0] * D)
    model = g.ArmModel(arm, [g.BodySphere(l, 0.05, (x, 0, 0)) for l in range(D) for x in (-0.45 / D, 0.0)])
    d = datasets.generate2Ddataset("TwoObstaclesDataset")
    fld = datasets.signedDistanceField2D(d.map, d.cell_size)
    st = TrajOptimizerSetting(D)
    st.set_total_step(N); st.set_total_time(3.0); st.set_obs_check_inter(2); st.set_cost_sigma(0.1); st.set_epsilon(0.2)
    st.set_conf_prior_model(1e-3); st.set_vel_prior_model(1e-3); st.set_Qc_model(np.eye(D)); st.set_max_iter(12)
    {"GN": st.setGaussNewton, "LM": st.setLM}[opt]()
    rng = np.random.default_rng(42)
    start = np.zeros((B, D))
    end = np.linspace(0.3, 0.9, D)[None] + 0.2 * rng.normal(size=(B, D))
    end[ALREADY_OPTIMAL_ROW] = 0.0      # at rest in free space from start to end: every factor's error is exactly 0
    init = np.stack([initArmTrajStraightLine(start[b], end[b], N) for b in range(B)])
    z = np.zeros((B, D))
    return problems.Problem(f"planar arm D={D} N={N} {opt}", model, [d.origin_x, d.origin_y], d.cell_size, fld, st, start,
                            z, end, z.copy(), init)


WAM_REST = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])     # upright above the desk: no sphere within epsilon of it


def wam(N, opt):
    p = problems.wam_restarts(B=B, total_step=N, obs_check_inter=2, opt=opt, sdf="40", max_iter=12)
    r = ALREADY_OPTIMAL_ROW
    p.start_conf[r] = p.end_conf[r] = WAM_REST
    p.init[r] = initArmTrajStraightLine(WAM_REST, WAM_REST, N)
    return p


def cases():
    out = {f"planar{D}_N11_GN": (lambda D=D: planar(D, 11, "GN")) for D in (1, 2, 3, 4)}
    out["planar2_N11_LM"] = lambda: planar(2, 11, "LM")
    for N in (21, 22, 43):
        for opt in ("GN", "LM"):
            out[f"planar2_N{N}_{opt}"] = lambda N=N, opt=opt: planar(2, N, opt)
    out["planar3_N43_LM"] = lambda: planar(3, 43, "LM")
    out["wam_N11_GN"] = lambda: wam(11, "GN")
    out["wam_N43_GN"] = lambda: wam(43, "GN")
    out["wam_N43_LM"] = lambda: wam(43, "LM")
    return out


UPDATE_CASES = ("planar2_N43_GN", "wam_N43_GN")       # also run as a fixed-iteration plan


def _raw_digests(engine, pl, nb, N):
    groups = (N + 1) // 4 + 1                          # as handover_cases.run_case
    count = {"tiles": nb * (N + 1) * 256, "fac": nb * (N + 1) * 768, "pend": nb * groups * 256, "coup": nb * groups * 256}
    raw = {}
    for name, which in hc.RAW.items():
        a = np.zeros(count[name])
        engine._ck(engine.lib.gpmp2mi_plan_debug_read(pl.h.ptr, which, a.ctypes.data_as(C.POINTER(C.c_double)),
                                                      C.c_long(a.size)))
        raw[name] = hc._digest(a)
    return raw


def run_linearize(engine, make):
    """gpmp2mi_plan_linearize at the initial trajectories -> {"lin_g", "lin_err"} and, under "lin_digest", the SHA-256 of
    Hdiag and Hoff"""
    p = make()
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pl = engine.plan(r, s, p.setting, p.init.shape[0])
    try:
        pl.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
        Hd, Ho, gv, err = pl.linearize(p.init)
    finally:
        pl.close()
    return {"lin_g": gv, "lin_err": err, "lin_digest": {"Hdiag": hc._digest(Hd), "Hoff": hc._digest(Ho)}}


def run_update(engine, make):
    """UPDATE_ITERATIONS fixed Gauss-Newton iterations (gpmp2mi_plan_update) -> as handover_cases.run_case"""
    p = make()
    nb, N = p.init.shape[0], p.init.shape[1] - 1
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pl = engine.plan(r, s, p.setting, nb)
    try:
        pl.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
        pl.update(UPDATE_ITERATIONS)
        res = pl.result()
        out = {k: np.array(res[k]) for k in RESULT_KEYS}
        out["raw"] = _raw_digests(engine, pl, nb, N)
    finally:
        pl.close()
    return out
