"""Time of re-timing a solved plan (include/gpmp2mi.h "re-timing") against the same answer over the host.  New paths:
Plan.retime_dev into device buffers + a wait, Plan.retime (host arrays), Plan.select_retimed_dev + a wait; beside them
Plan.motion_score_dev + a wait (the stage whose tiling k_retime_caps has).  Host route: result() -> sphere_centers with
Jacobians -> numpy caps -> the rule on one host thread, once as csrc/retime_rule.h built by the host compiler (every row)
and once as the numpy rule of tests/retime_reference.py (--numpy-rows rows, reported per row).  The headline problem (WAM
restarts, N = 100, inter_step 5) at B = 64 and 1 024, after optimize.

Every size is measured in a process of its own, started here under a time limit; the first one that fails ends the run.
Per variant the median and min / max of the per-call time over --windows windows of >= --window seconds, variants
alternated in one process, every shape warmed.  Kernel times come from a `rocprofv3 --kernel-trace --stats` run of their
own (a child process per size, --trace); the per-stage time of k_retime is its kernel time over the 2 (Md - 1) dependent
stages of a row.  No threshold is set: the table is the result.  Writes profiles/retime_throughput.txt.

usage: python scripts/retime_throughput.py [--window 0.5] [--windows 5] [--limit 420] [--out profiles/retime_throughput.txt]"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = (64, 1024)
VEL, ACC, POINT_SPEED, MAX_RATE = 2.0, 20.0, 1.5, 2.0
J = 5
CHUNK = 32768     # configurations per sphere_centers call of the host route: 3 S D doubles of Jacobian each


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


def host_inputs(eng, pl, r, dt):
    """result() -> per row (qd, qL, qR, cap, h) and ps, through the entry points that existed before"""
    import retime_reference as rr
    from gpmp2_amd._capi import dptr
    traj = pl.result()["traj"]
    B, D, S = traj.shape[0], r.dof, r.S
    up = eng.interpolate_traj(D, False, None, dt, J, traj)
    q, v = np.ascontiguousarray(up[:, :, :D]).reshape(-1, D), up[:, :, D:].reshape(-1, D)
    ps = np.zeros(q.shape[0])
    for i in range(0, q.shape[0], CHUNK):
        qc = np.ascontiguousarray(q[i:i + CHUNK])
        c, Jc = np.zeros((qc.shape[0], S, 3)), np.zeros((qc.shape[0], S, 3, D))
        eng._ck(eng.lib.gpmp2mi_sphere_centers(r.ptr, qc.shape[0], dptr(qc), dptr(c), dptr(Jc)))
        u = np.einsum("msid,md->msi", Jc, v[i:i + CHUNK])
        ps[i:i + CHUNK] = np.sqrt((u * u).sum(axis=2)).max(axis=1)
    ps = ps.reshape(B, -1)
    rows = []
    for b in range(B):
        qd, qL, qR, h = rr.path_from_traj(traj[b], dt, J)
        rows.append((qd, qL, qR, rr.rate_caps(qd, np.full(D, VEL), ps[b], POINT_SPEED), h))
    return rows, ps


def over_the_host(eng, pl, r, dt):
    """every row through the rule built by the host compiler, one thread"""
    import retime_shim
    rows, _ = host_inputs(eng, pl, r, dt)
    acc = np.full(r.dof, ACC)
    return np.array([retime_shim.retime_path(qd, qL, qR, cap, acc, h, MAX_RATE)["duration"] for qd, qL, qR, cap, h in rows])


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


def solved_plan(B):
    from gpmp2_amd import engine, problems
    eng = engine.Engine()
    p = problems.wam_restarts(B=B, total_step=100, obs_check_inter=5)
    r, s = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pl = eng.plan(r, s, p.setting, p.B)
    pl.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
    pl.optimize()
    lim = engine.MotionLimits(7, vel=VEL, acc=ACC, point_speed=POINT_SPEED)
    return eng, p, r, pl, lim


def trace(B, calls):
    """the child of the rocprofv3 run: nothing but `calls` re-timings of the solved plan"""
    eng, p, r, pl, lim = solved_plan(B)
    for _ in range(calls):
        pl.retime(lim, J, max_rate=MAX_RATE, out={"duration": np.zeros(B)})
    pl.close()
    return 0


def kernel_times(B, limit):
    """{kernel: (calls, average us, min us, max us)} of the two re-timing kernels from a rocprofv3 run of its own, or a
    reason why there is none"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d,
               "--", sys.executable, os.path.abspath(__file__), "--trace", str(B)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True)
        except OSError as e:
            return f"not measured (rocprofv3: {e})"
        if r.returncode != 0:
            return f"not measured (rocprofv3 run: exit status {r.returncode})"
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for row in csv.DictReader(fh):
                    if "k_retime" in row["Name"]:
                        name = "k_retime_caps" if "k_retime_caps" in row["Name"] else "k_retime"
                        out[name] = (int(row["Calls"]), float(row["AverageNs"]) / 1e3, float(row["MinNs"]) / 1e3,
                                     float(row["MaxNs"]) / 1e3)
        return out or "not measured (no k_retime row in the kernel statistics)"


def measure(B, window, count, numpy_rows, limit):
    import retime_reference as rr
    eng, p, r, pl, lim = solved_plan(B)
    N, D = p.setting.total_step, 7
    Md = N * (J + 1) + 1
    dt = p.setting.total_time / N
    f = lambda *shape: DevArray(eng, shape, np.float64)
    i = lambda *shape: DevArray(eng, shape, np.int32)
    o = dict(sdot=f(B, Md), u=f(B, Md), stamps=f(B, Md), duration=f(B), status=i(B), achieved=f(B, 4))
    mo = dict(pos_margin=f(B), vel_ratio=f(B), acc_ratio=f(B), point_speed=f(B), time_scale=f(B), worst=i(B, 4, 2), invalid=i(B))
    best, n, dur, sb, tb, db = i(1), i(1), f(1), f(Md), f(N + 1, 2 * D), f(Md, 2 * D)
    wait = lambda: eng._ck(eng.lib.gpmp2mi_debug_device_read(best.host.ctypes.data_as(C.c_void_p), best.p, C.c_size_t(4)))
    ptrs, mptrs = {k: a.ptr for k, a in o.items()}, {k: a.ptr for k, a in mo.items()}

    def retime_dev():
        pl.retime_dev(lim, J, max_rate=MAX_RATE, **ptrs)
        wait()

    def select_dev():
        pl.select_retimed_dev(J, lim, -np.inf, np.inf, MAX_RATE, None, None, 0.0, False, None, 0.0, best.ptr, n.ptr, dur.ptr,
                              sb.ptr, tb.ptr, db.ptr)
        wait()

    def motion_dev():
        pl.motion_score_dev(lim, J, **mptrs)
        wait()
    new = pl.retime(lim, J, max_rate=MAX_RATE)
    old = over_the_host(eng, pl, r, dt)
    retime_dev()
    agree = bool(np.allclose(new["duration"], old, rtol=1e-9, atol=0)) and \
        all(np.array_equal(o[k].read(), new[k], equal_nan=True) for k in o)
    scale = pl.motion_score(lim, J)["time_scale"]
    total = p.setting.total_time
    t = windows({"retime_dev_wait": retime_dev, "retime": lambda: pl.retime(lim, J, max_rate=MAX_RATE),
                 "select_retimed_dev_wait": select_dev, "motion_score_dev_wait": motion_dev,
                 "over_the_host": lambda: over_the_host(eng, pl, r, dt)}, window, count, wait)
    rows, _ = host_inputs(eng, pl, r, dt)
    t0 = time.perf_counter()
    for qd, qL, qR, cap, h in rows[:numpy_rows]:
        rr.retime_path(qd, qL, qR, cap, np.full(D, ACC), h, MAX_RATE)
    numpy_row = (time.perf_counter() - t0) / max(1, min(numpy_rows, B))
    row = dict(B=B, N=N, inter_step=J, spheres=r.S, checked_states=Md, stages_per_row=2 * (Md - 1), agrees_with_host=agree,
               status_ok=int((new["status"] == 0).sum()),
               uniform_duration=[float((np.maximum(scale, 1.0 / MAX_RATE) * total).min()), float((np.maximum(scale, 1.0 / MAX_RATE) * total).max())],
               retimed_duration=[float(new["duration"].min()), float(new["duration"].max())],
               retimed_over_uniform=[float((new["duration"] / (np.maximum(scale, 1.0 / MAX_RATE) * total)).min()),
                                     float((new["duration"] / (np.maximum(scale, 1.0 / MAX_RATE) * total)).max())],
               numpy_rule_ms_per_row=round(1e3 * numpy_row, 3))
    for name, v in t.items():
        row[name + "_ms"] = dict(median=round(1e3 * statistics.median(v), 4), min=round(1e3 * min(v), 4),
                                 max=round(1e3 * max(v), 4))
    pl.close()
    row["kernels_us"] = kernel_times(B, limit)
    print(json.dumps(row), flush=True)
    return 0 if agree else 1


def report(rows, commit):
    lines = []
    for row in rows:
        lines.append(f"re-timing on the headline WAM plan: B = {row['B']}, N = {row['N']}, inter_step {row['inter_step']}, "
                     f"{row['checked_states']} checked states, {row['spheres']} spheres, max_rate {MAX_RATE}; commit {commit}")
        lines.append(f"{'call':<28}{'median ms':>12}{'min ms':>12}{'max ms':>12}")
        for k in ("retime_dev_wait", "retime", "select_retimed_dev_wait", "motion_score_dev_wait", "over_the_host"):
            v = row[k + "_ms"]
            lines.append(f"{k:<28}{v['median']:>12.4f}{v['min']:>12.4f}{v['max']:>12.4f}")
        lines.append(f"numpy rule on the host: {row['numpy_rule_ms_per_row']} ms per row ({row['B']} rows: "
                     f"{row['numpy_rule_ms_per_row'] * row['B']:.0f} ms, extrapolated); over_the_host is the same rule built by the host "
                     "compiler, every row, one thread, with the inputs fetched and ps from sphere_centers")
        k = row["kernels_us"]
        if isinstance(k, dict):
            for name, (calls, avg, lo, hi) in sorted(k.items()):
                lines.append(f"kernel {name:<20}{avg:>10.1f} us  [{lo:.1f} - {hi:.1f}], {calls} calls (rocprofv3 --kernel-trace --stats)")
            if "k_retime" in k:
                lines.append(f"k_retime per dependent stage: {1e3 * k['k_retime'][1] / row['stages_per_row']:.1f} ns "
                             f"({row['stages_per_row']} stages per row, one wavefront per row)")
        else:
            lines.append(f"kernel times: {k}")
        lines.append(f"rows that re-time OK: {row['status_ok']} of {row['B']}; uniform stretch {row['uniform_duration'][0]:.3f} - "
                     f"{row['uniform_duration'][1]:.3f} s, re-timed {row['retimed_duration'][0]:.3f} - {row['retimed_duration'][1]:.3f} s, "
                     f"ratio {row['retimed_over_uniform'][0]:.3f} - {row['retimed_over_uniform'][1]:.3f}; "
                     f"device and host route agree: {row['agrees_with_host']}")
        lines.append(json.dumps(row))
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--limit", type=int, default=420, help="seconds a size may take")
    ap.add_argument("--numpy-rows", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retime_throughput.txt"))
    ap.add_argument("--size", type=int, choices=SIZES, help="measure this size in this process")
    ap.add_argument("--trace", type=int, choices=SIZES, help="the child of the kernel trace: re-time this size and leave")
    a = ap.parse_args()
    if a.trace:
        return trace(a.trace, 20)
    if a.size:
        return measure(a.size, a.window, a.windows, a.numpy_rows, a.limit)
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True).stdout.strip()
    commit = (commit or os.environ.get("GPMP2MI_COMMIT", "unknown")) + (" + uncommitted changes" if dirty else "")
    rows = []
    for B in SIZES:   # a process and a time limit per size; the first failure ends the run
        r = subprocess.run(["timeout", "-k", "10", str(2 * a.limit), sys.executable, os.path.abspath(__file__), "--size", str(B),
                            "--window", str(a.window), "--windows", str(a.windows), "--numpy-rows", str(a.numpy_rows),
                            "--limit", str(a.limit)], capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        print(r.stdout, end="", flush=True)
        lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
        if lines:
            rows.append(json.loads(lines[-1]))
        if r.returncode != 0:
            print(f"# B = {B}: exit status {r.returncode}; stopped here", flush=True)
            break
    with open(a.out, "w") as fh:
        fh.write(report(rows, commit))
    return 0 if len(rows) == len(SIZES) else 1


if __name__ == "__main__":
    sys.exit(main())
