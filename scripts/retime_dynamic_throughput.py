"""Time of re-timing a solved plan under torque limits (include/gpmp2mi.h "re-timing under torque limits") next to
re-timing without them, of the same build: Plan.retime_dynamic_dev into device buffers + a wait, Plan.retime_dev + a wait,
Plan.select_retimed_dynamic_dev + a wait, Plan.torque_score_dev + a wait (the stage whose tiling k_retime_coef has).  Host
route: the numpy rule of tests/retime_dynamic_reference.py with coefficients from tests/torque_reference.py on one host
thread (--numpy-rows rows, reported per row).  The headline problem (WAM restarts, N = 100, inter_step 5, the
illustrative inertial table of gpmp2_amd/dynamics.py) at B = 64 and 1 024, after optimize.

Every size is measured in a process of its own, started here under a time limit; the first one that fails ends the run.
Per variant the median and min / max of the per-call time over --windows windows of >= --window seconds, variants
alternated in one process, every shape warmed.  Kernel times come from a `rocprofv3 --kernel-trace --stats` run of their
own (a child process per size, --trace).  The re-timed durations stand next to the uniform stretch
max(time_scale, torque_time_scale, 1 / max_rate) * T of the same rows.  No threshold is set: the table is the result.
Writes profiles/retime_dynamic_throughput.txt.

usage: python scripts/retime_dynamic_throughput.py [--window 0.5] [--windows 5] [--limit 420] [--out FILE]"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import re
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
VEL, ACC, POINT_SPEED, MAX_RATE = 2.0, 20.0, 1.5, 2.0      # the limits of scripts/retime_throughput.py
J = 5


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
    from gpmp2_amd import dynamics, engine, problems
    eng = engine.Engine()
    p = problems.wam_restarts(B=B, total_step=100, obs_check_inter=5)
    r, s = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pl = eng.plan(r, s, p.setting, p.B)
    pl.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
    pl.optimize()
    lim = engine.MotionLimits(7, vel=VEL, acc=ACC, point_speed=POINT_SPEED)
    t = dict(dynamics.illustrative_wam(), gravity=np.array([0.0, 0.0, -9.81]))
    dyn = eng.dynamics(r, t["mass"], t["com"], t["inertia"], t["gravity"], t["torque"])
    return eng, p, r, pl, lim, t, dyn


def trace(B, calls):
    """the child of the rocprofv3 run: nothing but `calls` re-timings of the solved plan, with and without torque rows"""
    eng, p, r, pl, lim, t, dyn = solved_plan(B)
    for _ in range(calls):
        pl.retime_dynamic(dyn, lim, J, max_rate=MAX_RATE, out={"duration": np.zeros(B)}, tau=False, coef=False)
        pl.retime(lim, J, max_rate=MAX_RATE, out={"duration": np.zeros(B)})
    pl.close()
    return 0


def kernel_times(B, limit):
    """{kernel: (calls, average us, min us, max us)} from a rocprofv3 run of its own, or a reason why there is none"""
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
                    m = re.search(r"\b(k_retime\w*)", row["Name"])
                    name = m.group(1) if m and "finish" not in m.group(1) else None
                    if name:
                        calls, avg, lo, hi = int(row["Calls"]), float(row["AverageNs"]) / 1e3, float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3
                        if name in out:      # several instances of one kernel: calls add, the average is weighted
                            c0, a0, l0, h0 = out[name]
                            calls, avg, lo, hi = c0 + calls, (c0 * a0 + calls * avg) / (c0 + calls), min(l0, lo), max(h0, hi)
                        out[name] = (calls, avg, lo, hi)
        return out or "not measured (no k_retime row in the kernel statistics)"


def numpy_rows(p, t, traj, dt, rows):
    """seconds per row of the host route: coefficients by the link-frame recursion, then the numpy rule, one thread"""
    import retime_dynamic_reference as dr
    from oracle import Oracle
    orc = Oracle()
    t0 = time.perf_counter()
    coef = dr.coefficients(orc, p.model, t, dt, J, traj[:rows])
    for b in range(min(rows, traj.shape[0])):
        dr.retime_dynamic_traj(traj[b], coef[b], t["torque"], dt, J, vel=np.full(7, VEL), acc=np.full(7, ACC), max_rate=MAX_RATE)
    return (time.perf_counter() - t0) / max(1, min(rows, traj.shape[0]))


def measure(B, window, count, n_numpy, limit):
    eng, p, r, pl, lim, t, dyn = solved_plan(B)
    N, D = p.setting.total_step, 7
    Md = N * (J + 1) + 1
    dt = p.setting.total_time / N
    f = lambda *shape: DevArray(eng, shape, np.float64)      # noqa: E731
    i = lambda *shape: DevArray(eng, shape, np.int32)        # noqa: E731
    o = dict(sdot=f(B, Md), u=f(B, Md), stamps=f(B, Md), duration=f(B), status=i(B), achieved=f(B, 6), tau_retimed=f(B, Md, D))
    po = dict(sdot=f(B, Md), u=f(B, Md), stamps=f(B, Md), duration=f(B), status=i(B), achieved=f(B, 4))
    to = dict(torque_ratio=f(B), static_ratio=f(B), torque_time_scale=f(B), worst=i(B, 3, 2), invalid=i(B))
    best, n, dur, sb, tau, tb, db = i(1), i(1), f(1), f(Md), f(Md, D), f(N + 1, 2 * D), f(Md, 2 * D)
    wait = lambda: eng._ck(eng.lib.gpmp2mi_debug_device_read(best.host.ctypes.data_as(C.c_void_p), best.p, C.c_size_t(4)))  # noqa: E731
    ptrs, pptrs, tptrs = ({k: a.ptr for k, a in x.items()} for x in (o, po, to))

    def dynamic_dev():
        pl.retime_dynamic_dev(dyn, lim, J, max_rate=MAX_RATE, **ptrs)
        wait()

    def plain_dev():
        pl.retime_dev(lim, J, max_rate=MAX_RATE, **pptrs)
        wait()

    def select_dev():
        pl.select_retimed_dynamic_dev(J, lim, dyn, -np.inf, np.inf, MAX_RATE, None, None, 0.0, False, None, 0.0, best.ptr,
                                      n.ptr, dur.ptr, sb.ptr, tau.ptr, tb.ptr, db.ptr)
        wait()

    def torque_dev():
        pl.torque_score_dev(dyn, J, **tptrs)
        wait()
    new = pl.retime_dynamic(dyn, lim, J, max_rate=MAX_RATE)
    plain = pl.retime(lim, J, max_rate=MAX_RATE)
    dynamic_dev()
    agree = all(np.array_equal(o[k].read(), new[k], equal_nan=True) for k in o)
    scale = np.maximum(pl.motion_score(lim, J)["time_scale"], pl.torque_score(dyn, J, tau=False)["torque_time_scale"])
    uniform = np.maximum(scale, 1.0 / MAX_RATE) * p.setting.total_time
    ok = new["status"] == 0
    tvar = windows({"retime_dynamic_dev_wait": dynamic_dev, "retime_dev_wait": plain_dev,
                    "select_retimed_dynamic_dev_wait": select_dev, "torque_score_dev_wait": torque_dev}, window, count, wait)
    per_row = numpy_rows(p, t, pl.result()["traj"], dt, n_numpy)
    span = lambda x: [float(np.min(x)), float(np.max(x))] if np.size(x) else [float("nan")] * 2      # noqa: E731
    row = dict(B=B, N=N, inter_step=J, checked_states=Md, stages_per_row=2 * (Md - 1), rows_per_stage=4 * D + 1,
               dev_form_agrees_with_host_form=agree, status_counts=[int((new["status"] == s).sum()) for s in range(5)],
               uniform_duration=span(uniform[ok]), retimed_duration=span(new["duration"][ok]),
               retimed_over_uniform=span(new["duration"][ok] / uniform[ok]),
               retimed_over_plain_retime=span(new["duration"][ok] / plain["duration"][ok]),
               largest_torque_ratio_after=float(np.max(new["achieved"][ok, 4])) if ok.any() else float("nan"),
               numpy_rule_ms_per_row=round(1e3 * per_row, 3))
    for name, v in tvar.items():
        row[name + "_ms"] = dict(median=round(1e3 * statistics.median(v), 4), min=round(1e3 * min(v), 4),
                                 max=round(1e3 * max(v), 4))
    pl.close()
    row["kernels_us"] = kernel_times(B, limit)
    print(json.dumps(row), flush=True)
    return 0 if agree else 1


def report(rows, commit):
    lines = []
    for row in rows:
        lines.append(f"re-timing under torque limits on the headline WAM plan: B = {row['B']}, N = {row['N']}, inter_step "
                     f"{row['inter_step']}, {row['checked_states']} checked states, {row['rows_per_stage']} rows per stage "
                     f"(k_retime: 15), max_rate {MAX_RATE}; commit {commit}")
        lines.append(f"{'call':<36}{'median ms':>12}{'min ms':>12}{'max ms':>12}")
        for k in ("retime_dynamic_dev_wait", "retime_dev_wait", "select_retimed_dynamic_dev_wait", "torque_score_dev_wait"):
            v = row[k + "_ms"]
            lines.append(f"{k:<36}{v['median']:>12.4f}{v['min']:>12.4f}{v['max']:>12.4f}")
        lines.append(f"numpy rule on one host thread, coefficients by the link-frame recursion included: "
                     f"{row['numpy_rule_ms_per_row']} ms per row ({row['B']} rows: {row['numpy_rule_ms_per_row'] * row['B']:.0f} ms, "
                     "extrapolated)")
        k = row["kernels_us"]
        if isinstance(k, dict):
            for name, (calls, avg, lo, hi) in sorted(k.items()):
                lines.append(f"kernel {name:<20}{avg:>10.1f} us  [{lo:.1f} - {hi:.1f}], {calls} calls (rocprofv3 --kernel-trace --stats)")
            for name in ("k_retime_dynamic", "k_retime"):
                if name in k:
                    lines.append(f"{name} per dependent stage: {1e3 * k[name][1] / row['stages_per_row']:.1f} ns "
                                 f"({row['stages_per_row']} stages per row, one wavefront per row)")
        else:
            lines.append(f"kernel times: {k}")
        lines.append(f"status counts (OK, BOUNDARY, EMPTY, INVALID, STATIC): {row['status_counts']}; of the OK rows: uniform stretch "
                     f"{row['uniform_duration'][0]:.3f} - {row['uniform_duration'][1]:.3f} s, re-timed {row['retimed_duration'][0]:.3f} - "
                     f"{row['retimed_duration'][1]:.3f} s, ratio {row['retimed_over_uniform'][0]:.3f} - {row['retimed_over_uniform'][1]:.3f}; "
                     f"against re-timing without torque rows {row['retimed_over_plain_retime'][0]:.3f} - "
                     f"{row['retimed_over_plain_retime'][1]:.3f}; largest torque ratio of a re-timed row "
                     f"{row['largest_torque_ratio_after']:.16g}; `_dev` and host form agree: {row['dev_form_agrees_with_host_form']}")
        lines.append(json.dumps(row))
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--limit", type=int, default=420, help="seconds a size may take")
    ap.add_argument("--numpy-rows", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retime_dynamic_throughput.txt"))
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
