"""Time of the torque-limit calls on a solved plan against the same answer over the host.  Measured:
Plan.select_dynamic_dev + a wait (the whole selection: obstacle, motion and torque stages, one finish), beside it
Plan.select_feasible_dev + a wait on the same plan (the selection without the torque stage: the difference is what the
stage costs; the units behind select_feasible are those of the parent commit, unchanged), and Plan.torque_score_dev + a
wait (k_torque and k_torque_finish alone).  Baseline: result() -> interpolate_traj -> the numpy inverse dynamics of
tests/torque_reference.py and the score rule, on one host thread.  The headline problem (WAM restarts, N = 100,
inter_step 5) at B = 64 and 1 024, after optimize, with the illustrative inertial table of gpmp2_amd/dynamics.py.

Every size is measured in a process of its own, started here under a time limit; the first one that fails ends the run.
Per variant the median and min / max of the per-call time over --windows windows of >= --window seconds, variants
alternated in one process, every shape warmed.  No ratio is promised: the table says what was measured.

usage: python scripts/torque_throughput.py [--window 0.5] [--windows 3] [--limit 300] [--out profiles/torque_throughput.txt]"""
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
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
SIZES = (64, 1024)
DOWN, UP = [-2.6, -2.0, -2.8, -0.9, -4.76, -1.6, -3.0], [2.6, 2.0, 2.8, 3.1, 1.24, 1.6, 3.0]
VEL, ACC, POINT_SPEED = 2.0, 20.0, 1.5


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


class _Interp:
    """the engine's interpolate_traj with the oracle's signature, for torque_reference.checked_inputs"""

    def __init__(self, eng):
        self.eng = eng

    def interpolate_traj(self, D, lie, Qc, dt, J, t):
        return self.eng.interpolate_traj(D, lie, Qc, dt, J, t)


def over_the_host(eng, pl, model, table, dt, J):
    import torque_reference as tr
    traj = pl.result()["traj"]
    s = tr.torque_from_inputs(model.fk_model(), table, *tr.checked_inputs(_Interp(eng), model.dof(), dt, J, traj))
    return {k: s[k] for k in ("torque_ratio", "static_ratio", "torque_time_scale")}


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
    from gpmp2_amd import dynamics, engine, problems
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
    table = dict(dynamics.illustrative_wam(), gravity=np.array([0.0, 0.0, -9.81]))
    dyn = eng.dynamics(r, table["mass"], table["com"], table["inertia"], table["gravity"], table["torque"])
    f = lambda *shape: DevArray(eng, shape, np.float64)
    i = lambda *shape: DevArray(eng, shape, np.int32)
    o = dict(torque_ratio=f(B), static_ratio=f(B), torque_time_scale=f(B), worst=i(B, 3, 2), invalid=i(B))
    best, n, ts, ub, tb, db = i(1), i(1), f(1), f(Md, D), f(N + 1, 2 * D), f(Md, 2 * D)
    wait = lambda: eng._ck(eng.lib.gpmp2mi_debug_device_read(best.host.ctypes.data_as(C.c_void_p), best.p, C.c_size_t(4)))
    ptrs = {k: a.ptr for k, a in o.items()}
    mts = 3.0

    def score_dev():
        pl.torque_score_dev(dyn, J, **ptrs)
        wait()

    def dynamic_dev():
        pl.select_dynamic_dev(J, lim, dyn, 0.0, mts, 0.0, False, None, 0.0, best.ptr, n.ptr, ts.ptr, ub.ptr, tb.ptr, db.ptr)
        wait()

    def feasible_dev():
        pl.select_feasible_dev(J, lim, 0.0, mts, 0.0, False, None, 0.0, best.ptr, n.ptr, ts.ptr, tb.ptr, db.ptr)
        wait()
    new = pl.torque_score(dyn, J, tau=False)
    old = over_the_host(eng, pl, p.model, table, dt, J)
    score_dev()
    agree = all(np.allclose(new[k], old[k], rtol=1e-9, atol=1e-12) for k in old) and \
        all(np.array_equal(o[k].read(), new[k]) for k in o)
    t = windows({"torque_score_dev_wait": score_dev, "select_dynamic_dev_wait": dynamic_dev,
                 "select_feasible_dev_wait": feasible_dev,
                 "over_the_host": lambda: over_the_host(eng, pl, p.model, table, dt, J)}, window, count, wait)
    row = dict(B=B, N=N, inter_step=J, checked_states=Md, agrees_with_host=bool(agree),
               torque_ratio_range=[float(new["torque_ratio"].min()), float(new["torque_ratio"].max())])
    for name, v in t.items():
        row[name + "_ms"] = dict(median=round(1e3 * statistics.median(v), 4), min=round(1e3 * min(v), 4),
                                 max=round(1e3 * max(v), 4))
    row["dynamic_minus_feasible_ms"] = round(row["select_dynamic_dev_wait_ms"]["median"] - row["select_feasible_dev_wait_ms"]["median"], 4)
    row["states_per_second_k_torque"] = round(B * Md / (1e-3 * row["torque_score_dev_wait_ms"]["median"]))
    print(json.dumps(row), flush=True)
    pl.close()
    return 0 if agree else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds a size may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "torque_throughput.txt"))
    ap.add_argument("--size", type=int, choices=SIZES, help="measure this size in this process")
    a = ap.parse_args()
    if a.size:
        return measure(a.size, a.window, a.windows)
    lines = ["# torque limits on a solved plan (WAM restarts, N = 100, inter_step 5, illustrative inertial table), per call, ms:",
             "# median [min .. max] over windows; *_dev_wait: the device form and a 4-byte read-back; over_the_host: result() ->",
             "# interpolate_traj -> numpy inverse dynamics and rule, one thread.  select_feasible's units are the parent commit's.",
             f"# {'B':>5s} {'variant':28s} {'median':>10s} {'min':>10s} {'max':>10s}"]
    done = 0
    for B in SIZES:   # a process and a time limit per size; the first failure ends the run
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--size", str(B),
                            "--window", str(a.window), "--windows", str(a.windows)], capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        rows = [x for x in r.stdout.splitlines() if x.startswith("{")]
        if rows:
            row = json.loads(rows[-1])
            for k, v in row.items():
                if k.endswith("_ms") and isinstance(v, dict):
                    lines.append(f"  {B:5d} {k[:-3]:28s} {v['median']:10.4f} {v['min']:10.4f} {v['max']:10.4f}")
            lines.append(f"  {B:5d} the torque stage in a selection (select_dynamic - select_feasible): {row['dynamic_minus_feasible_ms']:.4f} ms; "
                         f"k_torque alone: {row['states_per_second_k_torque']:.3g} checked states / s; agrees with the host: "
                         f"{row['agrees_with_host']}; over_the_host / select_dynamic: "
                         f"{row['over_the_host_ms']['median'] / row['select_dynamic_dev_wait_ms']['median']:.0f}x")
            done += 1
        if r.returncode != 0:
            lines.append(f"# B = {B}: exit status {r.returncode}; stopped here")
            break
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text)
    return 0 if done == len(SIZES) else 1


if __name__ == "__main__":
    sys.exit(main())
