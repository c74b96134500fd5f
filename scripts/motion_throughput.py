"""Time of the motion-limit calls on a solved plan against the same answers over the host.  New paths: Plan.motion_score_dev
into device buffers + a wait, Plan.motion_score (host arrays), Plan.select_feasible_dev + a wait; beside them
Plan.select_checked_dev + a wait, for the difference the motion stage adds to a selection.  Baseline: result() ->
interpolate_traj -> sphere_centers with Jacobians -> numpy (J v, margins, ratios, the two acceleration formulas, reduce).
The headline problem (WAM restarts, N = 100, inter_step 5) at B = 1, 64 and 1 024, after optimize.

Every size is measured in a process of its own, started here under a time limit; the first one that fails ends the run.
Per variant the median and min / max of the per-call time over --windows windows of >= --window seconds, variants
alternated in one process, every shape warmed.  A case is accepted when the new path's median is below the baseline's
minimum.  Writes profiles/motion_throughput.json (a list, one entry per size).

usage: python scripts/motion_throughput.py [--window 0.5] [--windows 5] [--limit 300] [--out profiles/motion_throughput.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (1, 64, 1024)
DOWN, UP = [-2.6, -2.0, -2.8, -0.9, -4.76, -1.6, -3.0], [2.6, 2.0, 2.8, 3.1, 1.24, 1.6, 3.0]
VEL, ACC, POINT_SPEED = 2.0, 20.0, 1.5
CHUNK = 32768     # configurations per sphere_centers call of the baseline: 3 S D doubles of Jacobian each


class DevArray:
    """a device buffer from the library's own HIP runtime (gpmp2mi_debug_device_*): no second runtime in the process"""

    def __init__(self, eng, shape, dtype):
        self.eng, self.host = eng, np.zeros(shape, dtype=dtype)
        self.p = C.c_void_p()
        eng._ck(eng.lib.gpmp2mi_debug_device_alloc(C.c_size_t(self.host.nbytes), 0, C.byref(self.p)))

    @property
    def ptr(self):
        return self.p.value

    def read(self):
        self.eng._ck(self.eng.lib.gpmp2mi_debug_device_read(self.host.ctypes.data_as(C.c_void_p), self.p,
                                                            C.c_size_t(self.host.nbytes)))
        return self.host.copy()


def over_the_host(eng, pl, r, dt, J):
    """the five values per row through the entry points that existed before"""
    from gpmp2_amd._capi import dptr
    traj = pl.result()["traj"]
    B, D, S = traj.shape[0], r.dof, r.S
    up = eng.interpolate_traj(D, False, None, dt, J, traj)
    q, v = np.ascontiguousarray(up[:, :, :D]).reshape(-1, D), up[:, :, D:].reshape(-1, D)
    speed = np.zeros((q.shape[0], S))
    for i in range(0, q.shape[0], CHUNK):
        qc = np.ascontiguousarray(q[i:i + CHUNK])
        c, Jc = np.zeros((qc.shape[0], S, 3)), np.zeros((qc.shape[0], S, 3, D))
        eng._ck(eng.lib.gpmp2mi_sphere_centers(r.ptr, qc.shape[0], dptr(qc), dptr(c), dptr(Jc)))
        u = np.einsum("msid,md->msi", Jc, v[i:i + CHUNK])
        speed[i:i + CHUNK] = np.sqrt((u * u).sum(axis=2))
    down, upl = np.asarray(DOWN), np.asarray(UP)
    margin = np.minimum(up[:, :, :D] - down, upl - up[:, :, :D]).min(axis=(1, 2))
    vel_ratio = (np.abs(up[:, :, D:]) / VEL).max(axis=(1, 2))
    x0, v0, x1, v1 = traj[:, :-1, :D], traj[:, :-1, D:], traj[:, 1:, :D], traj[:, 1:, D:]
    w = 6.0 / (dt * dt)
    a0 = w * (x1 - x0) - (4.0 * v0 + 2.0 * v1) / dt
    a1 = -(w * (x1 - x0)) + (2.0 * v0 + 4.0 * v1) / dt
    acc_ratio = np.maximum(np.abs(a0), np.abs(a1)).max(axis=(1, 2)) / ACC
    point_speed = speed.reshape(B, -1).max(axis=1)
    scale = np.maximum(np.maximum(vel_ratio, np.sqrt(acc_ratio)), point_speed / POINT_SPEED)
    return dict(pos_margin=margin, vel_ratio=vel_ratio, acc_ratio=acc_ratio, point_speed=point_speed, time_scale=scale)


def windows(variants, window, count, sync):
    out = {name: [] for name in variants}
    for fn in variants.values():    # warm every shape
        fn()
    sync()
    for _ in range(count):
        for name, fn in variants.items():
            calls, t0 = 0, time.perf_counter()
            while True:
                fn()
                calls += 1
                if time.perf_counter() - t0 >= window:
                    break
            out[name].append((time.perf_counter() - t0) / calls)
    return out


def measure(B, window, count):
    from gpmp2_amd import engine, problems
    eng = engine.Engine()
    J = 5
    p = problems.wam_restarts(B=B, total_step=100, obs_check_inter=5)
    r, s = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pl = eng.plan(r, s, p.setting, p.B)
    pl.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
    pl.optimize()
    N, D = p.setting.total_step, 7
    Md = N * (J + 1) + 1
    dt = p.setting.total_time / N
    lim = engine.MotionLimits(7, pos_down=DOWN, pos_up=UP, vel=VEL, acc=ACC, point_speed=POINT_SPEED)
    pairs = eng.generate_self_pairs(r, 2, np.zeros((1, 7)))
    f = lambda *shape: DevArray(eng, shape, np.float64)
    i = lambda *shape: DevArray(eng, shape, np.int32)
    o = dict(pos_margin=f(B), vel_ratio=f(B), acc_ratio=f(B), point_speed=f(B), time_scale=f(B), worst=i(B, 4, 2), invalid=i(B))
    best, n, ts, tb, db = i(1), i(1), f(1), f(N + 1, 2 * D), f(Md, 2 * D)
    wait = lambda: eng._ck(eng.lib.gpmp2mi_debug_device_read(best.host.ctypes.data_as(C.c_void_p), best.p, C.c_size_t(4)))
    ptrs = {k: a.ptr for k, a in o.items()}
    mts = 3.0

    def score_dev():
        pl.motion_score_dev(lim, J, **ptrs)
        wait()

    def feasible_dev():
        pl.select_feasible_dev(J, lim, 0.0, mts, 0.0, False, pairs, 0.0, best.ptr, n.ptr, ts.ptr, tb.ptr, db.ptr)
        wait()

    def checked_dev():
        pl.select_checked_dev(J, pairs, 0.0, False, 0.0, best.ptr, n.ptr, tb.ptr, db.ptr)
        wait()
    new = pl.motion_score(lim, J)
    old = over_the_host(eng, pl, r, dt, J)
    score_dev()
    agree = all(np.allclose(new[k], old[k], rtol=1e-9, atol=1e-12) for k in old) and \
        all(np.array_equal(o[k].read(), new[k]) for k in new)
    t = windows({"motion_score_dev_wait": score_dev, "motion_score": lambda: pl.motion_score(lim, J),
                 "select_feasible_dev_wait": feasible_dev, "select_checked_dev_wait": checked_dev,
                 "over_the_host": lambda: over_the_host(eng, pl, r, dt, J)}, window, count, wait)
    row = dict(B=B, N=N, inter_step=J, spheres=r.S, pairs=pairs.P, checked_states=Md, agrees_with_host=bool(agree),
               outside=int((new["pos_margin"] < 0).sum()), time_scale_range=[float(new["time_scale"].min()), float(new["time_scale"].max())])
    for name, v in t.items():
        row[name + "_ms"] = dict(median=round(1e3 * statistics.median(v), 4), min=round(1e3 * min(v), 4),
                                 max=round(1e3 * max(v), 4))
    base_min = row["over_the_host_ms"]["min"]
    row["accepted"] = {k: bool(row[k + "_ms"]["median"] < base_min) for k in ("motion_score_dev_wait", "motion_score")}
    row["feasible_minus_checked_ms"] = round(row["select_feasible_dev_wait_ms"]["median"] - row["select_checked_dev_wait_ms"]["median"], 4)
    print(json.dumps(row), flush=True)
    pl.close()
    return 0 if agree else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds a size may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_throughput.json"))
    ap.add_argument("--size", type=int, choices=SIZES, help="measure this size in this process")
    a = ap.parse_args()
    if a.size:
        return measure(a.size, a.window, a.windows)
    rows = []
    for B in SIZES:   # a process and a time limit per size; the first failure ends the run
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--size", str(B),
                            "--window", str(a.window), "--windows", str(a.windows)], capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        print(r.stdout, end="", flush=True)
        lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
        if lines:
            rows.append(json.loads(lines[-1]))
        if r.returncode != 0:
            print(f"# B = {B}: exit status {r.returncode}; stopped here", flush=True)
            break
    with open(a.out, "w") as fh:
        json.dump(rows, fh, indent=1)
        fh.write("\n")
    return 0 if len(rows) == len(SIZES) else 1


if __name__ == "__main__":
    sys.exit(main())
