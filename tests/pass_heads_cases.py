"""The runs of tests/test_gpu_pass_heads.py and what is recorded of each (shared with
scripts/record_pass_heads_golden.py, which writes the fixture on the GPU at the commit whose results are to be kept).

The heads of the three Gauss-Newton pass kernels (k_linearize_arm, k_assemble, k_gn_step_cr) decide, from a handful of
per-trajectory words, whether a workgroup works at all, and the tail of the pass-closing kernel counts the trajectories
that go on.  The cases are the smallest runs that reach every order in which those exits are taken, on the problems of
tests/handover_cases.py:
  planar2 N=8 GN           three trajectories, the last at its optimum: it leaves in pass 0 while the others iterate
  ... max_iter = 1         every trajectory stops at the pass cap
  ... update               a fixed-iteration plan_update round: its closing pass builds nothing
  ... LM, DOGLEG           the shared k_assemble on the trial-step path, and its Dogleg-retry exit
  planar2 N=2, N=16        no fused level 2; the first level-16 task of the step kernel
  wam N=11                 the 7-joint plan (k_linearize_arm with the arm's own instance)
  planar2 N=8 B=257        past ASM_WT_MAX_B: the plain-store instance of k_assemble
  queue 5 through 2        a queue run: k_queue_scan publishes the count, slots are reloaded at pass boundaries
"""
from __future__ import annotations

import numpy as np

import handover_cases as hc

RESULT_KEYS = ("traj", "final_error", "trace", "iters", "status")
UPDATE_ITERS = 2
BIG_B = 257
QUEUE_M, QUEUE_SLOTS = 5, 2


def _planar(N, opt, max_iter=None):
    p = hc.planar2(N, opt)
    if max_iter is not None:
        p.setting.set_max_iter(max_iter)
    return p


def _rows(p, idx):
    return [x[idx] for x in (p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)]


def _masked_trace(res):
    """error_trace up to each trajectory's last iteration; what lies beyond is not part of the result"""
    tr = np.array(res["error_trace"])
    it = np.asarray(res["iters"])
    keep = np.arange(tr.shape[1])[None, :] <= it[:, None]
    return np.where(keep, tr, 0.0)


def _collect(res, launches=None):
    out = {"traj": np.array(res["traj"]), "final_error": np.array(res["final_error"]), "trace": _masked_trace(res),
           "iters": np.array(res["iters"]), "status": np.array(res["status"])}
    out["launches"] = launches
    return out


def _plain(make, rows=None, update=0, timing=True):
    """optimize() of a plan (rows: the problem's rows repeated to that many trajectories); update > 0: followed by a
    plan_update round of that many fixed iterations, which is what is recorded"""
    def run(engine):
        p = make()
        idx = np.arange(p.init.shape[0] if rows is None else rows) % p.init.shape[0]
        r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
        pl = engine.plan(r, s, p.setting, len(idx))
        try:
            if timing:
                pl.enable_timing(True)
            pl.set_problem(*_rows(p, idx))
            pl.optimize()
            if update:
                pl.update(update)
            launches = {k: int(v["launches"]) for k, v in pl.timing().items()} if timing else None
            return _collect(pl.result(), launches)
        finally:
            pl.close()
    return run


def _queue(make):
    def run(engine):
        p = make()
        idx = np.arange(QUEUE_M) % p.init.shape[0]
        r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
        pl = engine.plan(r, s, p.setting, QUEUE_SLOTS)
        try:
            return _collect(pl.optimize_queue(*_rows(p, idx)))
        finally:
            pl.close()
    return run


def cases():
    """name -> run(engine) -> the RESULT_KEYS arrays and "launches" (timing's launch counts, or None)"""
    return {
        "planar2_N8_GN": _plain(lambda: _planar(8, "GN")),
        "planar2_N8_GN_maxiter1": _plain(lambda: _planar(8, "GN", 1)),
        "planar2_N8_GN_update": _plain(lambda: _planar(8, "GN"), update=UPDATE_ITERS),
        "planar2_N8_LM": _plain(lambda: _planar(8, "LM")),
        "planar2_N8_DOGLEG": _plain(lambda: _planar(8, "DOGLEG")),
        "planar2_N2_GN": _plain(lambda: _planar(2, "GN")),
        "planar2_N16_GN": _plain(lambda: _planar(16, "GN")),
        "wam_N11_GN": _plain(hc.wam_n11),
        "planar2_N8_GN_B257": _plain(lambda: _planar(8, "GN"), rows=BIG_B),
        "queue_5_through_2_GN": _queue(lambda: _planar(8, "GN")),
    }


# the cases whose launch counts follow the Gauss-Newton fast driver's rule, and the iteration cap of each run
GN_LAUNCH_CASES = {
    "planar2_N8_GN": 12, "planar2_N8_GN_maxiter1": 1, "planar2_N8_GN_update": UPDATE_ITERS, "planar2_N2_GN": 12,
    "planar2_N16_GN": 12, "wam_N11_GN": 12, "planar2_N8_GN_B257": 12,
}
