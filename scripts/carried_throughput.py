"""Cost of the carried object of a plan per pass (include/gpmp2mi.h "carried object"), on the headline WAM plan
(restarts, B = 64, N = 100, obs_check_inter 5), Gauss-Newton with --iters fixed iterations.

Plans: `none` (no capacity), `empty` (capacity 64, nothing set: nothing is launched for the factor), `A16` and `A64` (a
box of 16 / 64 spheres of 3 cm on the last link, epsilon 0.05, sigma 0.02), and `body64`: what a user had before, a new
robot handle with the 64 spheres appended as body spheres and a new plan on it (its creation time is recorded as well).
With --parent-root DIR (a checkout of the parent commit with its library built) `parent_none` is the parent's plan
without capacity, measured by a child process on that tree in lockstep with this one's windows.  The one condition:
`empty` measures the same as `parent_none` (as `none` where there is no parent tree), i.e. its median is not above the
other's by more than the spread (max - min) of the windows, for one evaluation pass and for the solve.

Two clocks per plan: one evaluation pass (Plan.graph_error: the linearization, the factor, the error reduction, B doubles
back) and a solve.  Per variant the median and min / max of the per-call time over --windows windows of >= --window
seconds, variants alternated, every shape warmed.  Plan.select_carried (one enqueue) is timed against the same answer
over the host: result() -> interpolate_traj -> forward_kinematics -> centres in numpy -> sdf_query -> the rule in numpy.
The time of k_carried_accumulate comes from one rocprofv3 --kernel-trace --stats run of its own, without counters.

usage: python scripts/carried_throughput.py [--window 0.5] [--windows 5] [--iters 10] [--parent-root DIR]
                                            [--out profiles/carried_throughput.txt]"""
import argparse
import copy
import csv
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
EPSILON, SIGMA, RADIUS, J = 0.05, 0.02, 0.03, 4

# the child on the parent's tree: a plan without capacity; one window of each clock per line read from stdin
_PARENT = r"""
import json, sys, time
from gpmp2_amd import engine, problems
window, iters = float(sys.argv[1]), int(sys.argv[2])
eng = engine.Engine()
p = problems.wam_restarts(B=64, total_step=100, obs_check_inter=5)
p.setting.fixed_iterations = iters
r, s = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
pl = eng.plan(r, s, p.setting, p.B)
args = (p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
pl.set_problem(*args)
def solve():
    pl.set_problem(*args)
    pl.optimize()
def one(fn):
    calls, t0 = 0, time.perf_counter()
    while True:
        fn()
        calls += 1
        if time.perf_counter() - t0 >= window:
            break
    pl.graph_error(p.init)
    return (time.perf_counter() - t0) / calls
pl.graph_error(p.init); solve()
print("ready", flush=True)
for line in sys.stdin:
    if line.strip() != "go":
        break
    print(json.dumps([one(lambda: pl.graph_error(p.init)), one(solve)]), flush=True)
"""


def box(A):
    """A spheres of 3 cm on a grid 8 .. 26 cm in front of the hand"""
    n, nz = {16: (2, 4), 64: (4, 4)}[A]
    g = np.meshgrid(np.linspace(-0.04, 0.04, n), np.linspace(-0.04, 0.04, n), np.linspace(0.08, 0.26, nz), indexing="ij")
    return np.full(A, RADIUS), np.ascontiguousarray(np.stack([x.ravel() for x in g], axis=1))


def make(iters):
    sys.path.insert(0, ROOT)
    from gpmp2_amd import engine, problems, robots
    eng = engine.Engine()
    p = problems.wam_restarts(B=64, total_step=100, obs_check_inter=5)
    p.setting.fixed_iterations = iters
    r, s = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    link = r.L - 1
    sets = {"A16": box(16), "A64": box(64)}

    def plan(capacity, key=None, robot=r):
        st = copy.deepcopy(p.setting)
        if capacity:
            st.set_carried_spheres(capacity, EPSILON, SIGMA)
        pl = eng.plan(robot, s, st, p.B)
        if key:
            pl.set_carried(link, *sets[key])
        return pl

    plans = {"none": plan(0), "empty": plan(64), "A16": plan(64, "A16"), "A64": plan(64, "A64")}
    # the alternative: the spheres as body spheres of a new robot handle, a new plan on it
    t0 = time.perf_counter()
    rad, cen = sets["A64"]
    body = robots.RobotModel(p.model.fk_model(), list(p.model.spheres) +
                             [robots.BodySphere(link, float(a), tuple(c)) for a, c in zip(rad, cen)])
    rb = eng.robot(body)
    plans["body64"] = plan(0, robot=rb)
    created = time.perf_counter() - t0
    return eng, p, r, s, link, sets, plans, created


def trace(calls):
    """the child of the rocprofv3 run: nothing but `calls` evaluation passes of the plan that carries 64 spheres"""
    eng, p, r, s, link, sets, plans, _ = make(10)
    pl = plans["A64"]
    pl.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
    for _ in range(calls):
        pl.graph_error(p.init)
    return 0


def kernel_times(limit):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d,
               "--", sys.executable, os.path.abspath(__file__), "--trace"]
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
                    if "k_carried_accumulate" in row["Name"]:
                        out["k_carried_accumulate"] = (int(row["Calls"]), float(row["AverageNs"]) / 1e3,
                                                       float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3)
        return out or "not measured (no row of the kernel in the kernel statistics)"


def host_select(eng, r, s, pl, p, link, rad, cen, dt):
    """the answer of select_carried(-inf thresholds but the carried clearance >= 0) over the host"""
    from gpmp2_amd import scoring
    res = pl.result()
    D = r.dof
    U = eng.interpolate_traj(D, False, None, dt, J, res["traj"])
    B, Md = U.shape[0], U.shape[1]
    poses, _ = eng.forward_kinematics(r, np.ascontiguousarray(U[:, :, :D]).reshape(-1, D))
    T = poses[:, link]
    c = np.einsum("mij,aj->mai", T[:, :3, :3], cen) + T[:, None, :3, 3]
    d, _, inr = eng.sdf_query(s, c.reshape(-1, 3))
    clr = np.where(inr.astype(bool), d - np.tile(rad, B * Md), np.inf).reshape(B, -1).min(axis=1)
    return scoring.carried_rule(res["final_error"], res["status"], np.full(B, np.inf), np.zeros(B, dtype=np.int32), -np.inf,
                                False, min_carried_clearance=clr, required_carried_clearance=0.0)


def measure(window, count, iters, limit, parent_root):
    eng, p, r, s, link, sets, plans, created = make(iters)
    args = (p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
    for pl in plans.values():
        pl.set_problem(*args)

    def solve(pl):
        pl.set_problem(*args)
        pl.optimize()

    v = {}
    for name, pl in plans.items():
        v["graph_error_" + name] = lambda pl=pl: pl.graph_error(p.init)
        v["solve_" + name] = lambda pl=pl: solve(pl)
    pa = plans["A64"]
    solve(pa)
    dt = p.setting.total_time / p.setting.total_step
    rad, cen = sets["A64"]
    dev = pa.select_carried(J, 0.0, required_clearance=-np.inf)
    host = host_select(eng, r, s, pa, p, link, rad, cen, dt)
    v["select_carried_device"] = lambda: pa.select_carried(J, 0.0, required_clearance=-np.inf)
    v["select_carried_host"] = lambda: host_select(eng, r, s, pa, p, link, rad, cen, dt)
    first = plans["none"]
    sync = lambda: first.graph_error(p.init)
    child = None
    if parent_root:
        env = dict(os.environ, PYTHONPATH=parent_root)
        child = subprocess.Popen([sys.executable, "-c", _PARENT, str(window), str(iters)], stdin=subprocess.PIPE,
                                 stdout=subprocess.PIPE, text=True, cwd=parent_root, env=env)
        assert child.stdout.readline().strip() == "ready"
    out = {name: [] for name in v}
    parent = {"graph_error_parent_none": [], "solve_parent_none": []}
    for fn in v.values():    # warm every shape
        fn()
    sync()
    for _ in range(count):
        for name, fn in v.items():
            calls, t0 = 0, time.perf_counter()
            while True:
                fn()
                calls += 1
                if time.perf_counter() - t0 >= window:
                    break
            sync()
            out[name].append((time.perf_counter() - t0) / calls)
        if child:
            child.stdin.write("go\n")
            child.stdin.flush()
            a, b = json.loads(child.stdout.readline())
            parent["graph_error_parent_none"].append(a)
            parent["solve_parent_none"].append(b)
    if child:
        child.stdin.write("end\n")
        child.stdin.close()
        child.wait(timeout=60)
        out.update(parent)
    row = dict(B=p.B, N=p.setting.total_step, dof=r.dof, fixed_iterations=iters, body64_created_ms=round(1e3 * created, 2),
               select_agrees=bool((dev["best"], dev["n_eligible"]) == tuple(host)), select=[dev["best"], dev["n_eligible"]])
    for name, x in out.items():
        row[name + "_ms"] = dict(median=round(1e3 * statistics.median(x), 4), min=round(1e3 * min(x), 4), max=round(1e3 * max(x), 4))
    for pl in plans.values():
        pl.close()
    row["kernels_us"] = kernel_times(limit)
    return row


def report(row, commit, window, count):
    lines = [f"carried object in a plan, WAM: B = {row['B']}, N = {row['N']}, dof {row['dof']}, GN x{row['fixed_iterations']}, "
             f"{count} windows of {window} s; commit {commit}",
             f"{'call':<30}{'median ms':>12}{'min ms':>12}{'max ms':>12}"]
    for k in [k[:-3] for k in row if k.endswith("_ms") and isinstance(row[k], dict)]:
        x = row[k + "_ms"]
        lines.append(f"{k:<30}{x['median']:>12.4f}{x['min']:>12.4f}{x['max']:>12.4f}")
    med = lambda k: row[k + "_ms"]["median"]
    spread = lambda k: row[k + "_ms"]["max"] - row[k + "_ms"]["min"]
    base = "parent_none" if "graph_error_parent_none_ms" in row else "none"
    ok_all = True
    for k in ("graph_error", "solve"):
        new, old = f"{k}_empty", f"{k}_{base}"
        sp = max(spread(new), spread(old))
        ok = med(new) <= med(old) + sp
        ok_all = ok_all and ok
        lines.append(f"the condition, {k}: empty {med(new):.4f} ms against {base} {med(old):.4f} ms, spread of the windows "
                     f"{sp:.4f} ms: {'met' if ok else 'NOT met'}")
    passes = row["fixed_iterations"] + 1
    lines.append(f"against `empty`, per evaluation pass: A16 {1e3 * (med('graph_error_A16') - med('graph_error_empty')):.1f} us, "
                 f"A64 {1e3 * (med('graph_error_A64') - med('graph_error_empty')):.1f} us, body64 "
                 f"{1e3 * (med('graph_error_body64') - med('graph_error_empty')):.1f} us; per solver pass ({passes} per solve): "
                 f"A16 {1e3 * (med('solve_A16') - med('solve_empty')) / passes:.1f} us, A64 "
                 f"{1e3 * (med('solve_A64') - med('solve_empty')) / passes:.1f} us, body64 "
                 f"{1e3 * (med('solve_body64') - med('solve_empty')) / passes:.1f} us (different problems: the solves are shown as measured)")
    lines.append(f"the alternative (a new robot handle with 64 more body spheres and a new plan): created in "
                 f"{row['body64_created_ms']:.1f} ms, once per grasp; Plan.set_carried is two copies")
    lines.append(f"select_carried: device {med('select_carried_device'):.4f} ms, over the host {med('select_carried_host'):.4f} ms; "
                 f"the same answer {row['select']}: {row['select_agrees']}")
    k = row["kernels_us"]
    if isinstance(k, dict):
        for name, (calls, avg, lo, hi) in sorted(k.items()):
            lines.append(f"kernel {name:<24}{avg:>10.1f} us  [{lo:.1f} - {hi:.1f}], {calls} calls (rocprofv3 --kernel-trace --stats, "
                         "evaluation passes of the plan with 64 spheres)")
    else:
        lines.append(f"kernel times: {k}")
    lines.append(json.dumps(row))
    return "\n".join(lines) + "\n", ok_all


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--limit", type=int, default=200, help="seconds the kernel trace may take")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "carried_throughput.txt"))
    ap.add_argument("--trace", action="store_true", help="the child of the kernel trace: evaluate and leave")
    a = ap.parse_args()
    if a.trace:
        return trace(20)
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True).stdout.strip()
    commit = (commit or os.environ.get("GPMP2MI_COMMIT", "unknown")) + (" + uncommitted changes" if dirty else "")
    row = measure(a.window, a.windows, a.iters, a.limit, a.parent_root)
    text, ok = report(row, commit, a.window, a.windows)
    print(text, end="")
    with open(a.out, "w") as fh:
        fh.write(text)
    return 0 if ok and row["select_agrees"] else 1


if __name__ == "__main__":
    sys.exit(main())
