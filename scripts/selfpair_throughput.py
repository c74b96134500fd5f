"""Cost of the self-collision table of a plan per pass (include/gpmp2mi.h "self-collision table in a plan").

Two workloads, each measured in a process of its own under its own time limit; the first failure ends the run:
  wam   the headline WAM plan (restarts, B = 64, N = 100, obs_check_inter 5), Gauss-Newton with --iters fixed iterations.
        Plans: `none` (no capacity), `empty` (capacity 78, nothing set: nothing is launched for the factor), `table78` (the
        78 generated pairs at (0.05, 0.005)), `table16` (the 16 pairs that come closest on the initial values, at
        (0.05, 0.02), through the table) and `rows16` (the same 16 rows through gpmp2mi_graph_opts::n_self_collision, the
        route that existed before: stored rows, k_self_collision + k_extra_accumulate).  `rows16` is the baseline of
        `table16`: the condition is that the table's median is not above the rows' median by more than the spread
        (max - min) of the windows.
  pr2   tests/score_reference.py::pr2_problem (dof 18, 65 spheres, N = 50, LM to tolerance, B = 4) with its generated table
        of more than 1 000 pairs, `empty` against `table`.
Two clocks per plan: one evaluation pass (Plan.graph_error: the linearization, the factor, the error reduction, B doubles
back) and a solve.  Per variant the median and min / max of the per-call time over --windows windows of >= --window
seconds, variants alternated in one process, every shape warmed.  The kernel times of k_sphere_centers and
k_selfpair_accumulate come from one rocprofv3 --kernel-trace --stats run per workload, of its own, without counters.

usage: python scripts/selfpair_throughput.py [--window 0.5] [--windows 5] [--iters 10] [--out profiles/selfpair_throughput.txt]"""
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
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
EPSILON, SIGMA, SIGMA16 = 0.05, 0.005, 0.02
CASES = ("wam", "pr2")


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
            sync()
            out[name].append((time.perf_counter() - t0) / calls)
    return out


def closest_sixteen(eng, r, p, table):
    """the 16 rows of `table` whose pairs come closest on the initial values, at (EPSILON, SIGMA16)"""
    c, _ = eng.sphere_centers(r, np.ascontiguousarray(p.init[:, :, :r.dof]).reshape(-1, r.dof))
    radius = np.asarray(p.model.flat()["sphere_radius"], dtype=np.float64)
    a, b = table[:, 0].astype(int), table[:, 1].astype(int)
    clr = np.sqrt(((c[:, a] - c[:, b]) ** 2).sum(axis=2)) - (radius[a] + radius[b])
    t = table[np.sort(np.argsort(clr.min(axis=0), kind="stable")[:16])].copy()
    t[:, 2], t[:, 3] = EPSILON, SIGMA16
    return t


def plans_of(case, iters):
    """(engine, problem, {name: plan with its table set})"""
    from gpmp2_amd import engine, problems
    eng = engine.Engine()
    if case == "wam":
        p = problems.wam_restarts(B=64, total_step=100, obs_check_inter=5)
        p.setting.fixed_iterations = iters
    else:
        import score_reference
        p = score_reference.pr2_problem(4)
    r, s = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    full = eng.generate_self_pairs(r, 2, np.zeros((1, r.dof)), EPSILON, SIGMA)

    def plan(capacity, table=None, rows=None):
        st = copy.deepcopy(p.setting)
        if capacity:
            st.set_self_pairs(capacity)
        if rows is not None:
            st.self_collision = rows
        pl = eng.plan(r, s, st, p.B)
        if table is not None:
            h = eng.self_pairs(r, table)
            pl.set_self_pairs(h)
            h.close()
        return pl

    if case == "wam":
        t16 = closest_sixteen(eng, r, p, full.data)
        plans = {"none": plan(0), "empty": plan(full.P), "table78": plan(full.P, full.data), "table16": plan(16, t16),
                 "rows16": plan(0, rows=t16)}
    else:
        plans = {"empty": plan(full.P), "table": plan(full.P, full.data)}
    return eng, p, r, plans, full.P


def trace(case, calls):
    """the child of the rocprofv3 run: nothing but `calls` evaluation passes of the plan that carries the full table"""
    eng, p, r, plans, P = plans_of(case, 10)
    pl = plans["table78" if case == "wam" else "table"]
    pl.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
    for _ in range(calls):
        pl.graph_error(p.init)
    return 0


def kernel_times(case, limit):
    """{kernel: (calls, average us, min us, max us)} of k_sphere_centers and k_selfpair_accumulate from a rocprofv3 run
    of its own, or a reason why there is none"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d,
               "--", sys.executable, os.path.abspath(__file__), "--trace", case]
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
                    for name in ("k_sphere_centers", "k_selfpair_accumulate"):
                        if name in row["Name"]:
                            out[name] = (int(row["Calls"]), float(row["AverageNs"]) / 1e3, float(row["MinNs"]) / 1e3,
                                         float(row["MaxNs"]) / 1e3)
        return out or "not measured (no row of the two kernels in the kernel statistics)"


def measure(case, window, count, iters, limit):
    eng, p, r, plans, P = plans_of(case, iters)
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
    first = next(iter(plans.values()))
    t = windows(v, window, count, lambda: first.graph_error(p.init))
    row = dict(case=case, B=p.B, N=p.setting.total_step, dof=r.dof, spheres=r.S, pairs=P,
               fixed_iterations=p.setting.fixed_iterations, iters={})
    for name, pl in plans.items():
        solve(pl)
        it = pl.result()["iters"]
        row["iters"][name] = [int(it.min()), int(it.max())]
    if case == "wam":
        a, b = plans["table16"].result(), plans["rows16"].result()
        row["routes_agree"] = bool(np.abs(a["traj"] - b["traj"]).max() <= 1e-6 and list(a["iters"]) == list(b["iters"]))
    for name, x in t.items():
        row[name + "_ms"] = dict(median=round(1e3 * statistics.median(x), 4), min=round(1e3 * min(x), 4), max=round(1e3 * max(x), 4))
    for pl in plans.values():
        pl.close()
    row["kernels_us"] = kernel_times(case, limit)
    print(json.dumps(row), flush=True)
    return 0 if row.get("routes_agree", True) else 1


def report(rows, commit, window, count):
    lines = []
    for row in rows:
        lines.append(f"self-collision table in a plan, {row['case']}: B = {row['B']}, N = {row['N']}, dof {row['dof']}, "
                     f"{row['spheres']} spheres, {row['pairs']} generated pairs, {count} windows of {window} s; commit {commit}")
        lines.append(f"{'call':<26}{'median ms':>12}{'min ms':>12}{'max ms':>12}")
        names = [k[:-3] for k in row if k.endswith("_ms")]
        for k in names:
            x = row[k + "_ms"]
            lines.append(f"{k:<26}{x['median']:>12.4f}{x['min']:>12.4f}{x['max']:>12.4f}")
        lines.append(f"iterations (min, max) per plan: {row['iters']}")
        med = lambda k: row[k + "_ms"]["median"]
        spread = lambda k: row[k + "_ms"]["max"] - row[k + "_ms"]["min"]
        if row["case"] == "wam":
            passes = row["fixed_iterations"] + 1
            lines.append(f"against `empty`, per evaluation pass: table78 {1e3 * (med('graph_error_table78') - med('graph_error_empty')):.1f} us, "
                         f"table16 {1e3 * (med('graph_error_table16') - med('graph_error_empty')):.1f} us, rows16 "
                         f"{1e3 * (med('graph_error_rows16') - med('graph_error_empty')):.1f} us; per solver pass ({passes} per solve): "
                         f"table78 {1e3 * (med('solve_table78') - med('solve_empty')) / passes:.1f} us, table16 "
                         f"{1e3 * (med('solve_table16') - med('solve_empty')) / passes:.1f} us, rows16 "
                         f"{1e3 * (med('solve_rows16') - med('solve_empty')) / passes:.1f} us")
            lines.append(f"capacity alone (`empty` against `none`): evaluation pass {1e3 * (med('graph_error_empty') - med('graph_error_none')):+.1f} us, "
                         f"solve {1e3 * (med('solve_empty') - med('solve_none')):+.1f} us (a plan with capacity takes the path of plans "
                         "with extra factors: no early stop)")
            for k in ("graph_error", "solve"):
                new, old = k + "_table16", k + "_rows16"
                sp = max(spread(new), spread(old))
                ok = med(new) <= med(old) + sp
                lines.append(f"condition (c), {k}: table16 {med(new):.4f} ms against rows16 {med(old):.4f} ms (baseline: this commit's "
                             f"build of the existing route), spread of the windows {sp:.4f} ms: {'met' if ok else 'NOT met'}")
            lines.append(f"the two routes solve alike: {row['routes_agree']}")
        else:
            lines.append(f"against `empty`: evaluation pass {1e3 * (med('graph_error_table') - med('graph_error_empty')):.1f} us; the solves "
                         "are different problems (LM to tolerance), their times are shown as measured")
        k = row["kernels_us"]
        if isinstance(k, dict):
            for name, (calls, avg, lo, hi) in sorted(k.items()):
                lines.append(f"kernel {name:<24}{avg:>10.1f} us  [{lo:.1f} - {hi:.1f}], {calls} calls (rocprofv3 --kernel-trace --stats, "
                             "evaluation passes of the plan with the full table)")
        else:
            lines.append(f"kernel times: {k}")
        lines.append(json.dumps(row))
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--limit", type=int, default=200, help="seconds a workload, and its kernel trace, may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selfpair_throughput.txt"))
    ap.add_argument("--case", choices=CASES, help="measure this workload in this process")
    ap.add_argument("--trace", choices=CASES, help="the child of the kernel trace: evaluate this workload and leave")
    a = ap.parse_args()
    if a.trace:
        return trace(a.trace, 20)
    if a.case:
        return measure(a.case, a.window, a.windows, a.iters, a.limit)
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True).stdout.strip()
    commit = (commit or os.environ.get("GPMP2MI_COMMIT", "unknown")) + (" + uncommitted changes" if dirty else "")
    rows = []
    for case in CASES:   # a process and a time limit per workload; the first failure ends the run
        r = subprocess.run(["timeout", "-k", "10", str(2 * a.limit), sys.executable, os.path.abspath(__file__), "--case", case,
                            "--window", str(a.window), "--windows", str(a.windows), "--iters", str(a.iters),
                            "--limit", str(a.limit)], capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        print(r.stdout, end="", flush=True)
        lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
        if lines:
            rows.append(json.loads(lines[-1]))
        if r.returncode != 0:
            print(f"# {case}: exit status {r.returncode}; stopped here", flush=True)
            break
    with open(a.out, "w") as fh:
        fh.write(report(rows, commit, a.window, a.windows))
    return 0 if len(rows) == len(CASES) else 1


if __name__ == "__main__":
    sys.exit(main())
