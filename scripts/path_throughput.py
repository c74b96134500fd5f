"""Cost of the workspace-path factor per pass, and time of the path check against the same answer over the host.

The workload is the headline WAM plan (restarts, B = 64, N = 100, obs_check_inter 5).  Three plans of it:
  none      created with room for a path, no path set (nothing is launched for the factor);
  path      the same plan with a constant ORIENTATION target of the last link on all 101 states, carried by the fused
            k_path_accumulate (one wavefront per trajectory and state, no stored rows);
  factor    the same constraint as ONE existing workspace factor over states 0..N (forward kinematics of all links of all
            states, k_workspace_prior, k_extra_accumulate).
Both formulations are valid for a constant target; the script prints whether their solves agree.  Two clocks per variant:
one evaluation pass (Plan.graph_error: the linearization, the factor, the error reduction, B doubles back) and a
Gauss-Newton run of --iters fixed iterations; the factor's cost per pass is the difference to `none`.  The check:
Plan.select_path (inter_step 5) against result() -> interpolate_traj -> forward_kinematics -> numpy.

Per variant the median and min / max of the per-call time over --windows windows of >= --window seconds, variants
alternated, every shape warmed.  A table on stdout, closed by one JSON line; no ratio is asked for.

usage: python scripts/path_throughput.py [--window 0.5] [--windows 5] [--iters 10] > profiles/path_throughput.txt"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LINK, SIGMA, J, ORIENTATION = 6, 0.05, 5, 1


def rot_angle(Ra, Rb):
    """angle of Ra^T Rb, batched over the leading axes"""
    R = np.swapaxes(Ra, -1, -2) @ Rb
    s = 0.5 * np.sqrt((R[..., 2, 1] - R[..., 1, 2]) ** 2 + (R[..., 0, 2] - R[..., 2, 0]) ** 2 + (R[..., 1, 0] - R[..., 0, 1]) ** 2)
    return np.arctan2(s, 0.5 * (np.trace(R, axis1=-2, axis2=-1) - 1.0))


def over_the_host(eng, pl, r, hold, dt, obstacle, allowed):
    """the same pick through the entry points that existed before: two host round trips and a numpy reduce"""
    from gpmp2_amd import scoring
    res = pl.result()
    traj = res["traj"]
    B, D = traj.shape[0], r.dof
    up = eng.interpolate_traj(D, False, None, dt, J, traj)
    poses, _ = eng.forward_kinematics(r, np.ascontiguousarray(up[:, :, :D]).reshape(-1, D))
    dev = rot_angle(hold[:3, :3], poses[:, LINK, :3, :3]).reshape(B, -1)
    valid = np.isfinite(dev)
    mx = np.where(valid, dev, -np.inf).max(axis=1)
    best, n = scoring.path_rule(res["final_error"], res["status"], obstacle["min_clearance"], obstacle["out_of_range"], 0.0,
                                False, max_rot_dev=mx, path_invalid=(~valid).sum(axis=1), max_rot_dev_allowed=allowed)
    return dict(best=best, n_eligible=n, max_rot_dev=mx)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    from gpmp2_amd import engine, problems
    eng = engine.Engine()
    p = problems.wam_restarts(B=64, total_step=100, obs_check_inter=5)
    p.setting.fixed_iterations = a.iters
    N = p.setting.total_step
    r, s = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    hold = eng.forward_kinematics(r, p.start_conf[:1])[0][0, LINK]
    dt = p.setting.total_time / N
    args = (p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
    with_path, with_factor = copy.deepcopy(p.setting), copy.deepcopy(p.setting)
    with_path.set_workspace_path(ORIENTATION, LINK)
    with_factor.add_workspace_prior(ORIENTATION, LINK, hold, SIGMA, 0, N)
    plans = {"none": eng.plan(r, s, with_path, p.B), "path": eng.plan(r, s, with_path, p.B),
             "factor": eng.plan(r, s, with_factor, p.B)}
    plans["path"].set_workspace_path(np.repeat(hold[None], N + 1, 0), SIGMA)
    for pl in plans.values():
        pl.set_problem(*args)

    def solve(pl):
        pl.set_problem(*args)
        pl.optimize()

    solve(plans["path"])
    solve(plans["factor"])
    ra, rb = plans["path"].result(), plans["factor"].result()
    solves_agree = bool(np.abs(ra["traj"] - rb["traj"]).max() <= 1e-6 and list(ra["iters"]) == list(rb["iters"]) and
                        np.allclose(ra["final_error"], rb["final_error"], rtol=1e-8, atol=0))
    sync = lambda: plans["path"].graph_error(p.init)
    v = {}
    for name, pl in plans.items():
        v["graph_error_" + name] = lambda pl=pl: pl.graph_error(p.init)
        v["solve_" + name] = lambda pl=pl: solve(pl)
    t = windows(v, a.window, a.windows, sync)
    # the check and the selection, on the solution of the plan that carries the path
    pl = plans["path"]
    solve(pl)
    obstacle = pl.score(J)
    dev = pl.path_score(J)
    allowed = float(np.median(dev["max_rot_dev"]))
    new = pl.select_path(J, max_rot_dev_allowed=allowed)
    old = over_the_host(eng, pl, r, hold, dt, obstacle, allowed)
    check_agrees = bool((new["best"], new["n_eligible"]) == (old["best"], old["n_eligible"]) and
                        np.allclose(dev["max_rot_dev"], old["max_rot_dev"], rtol=0, atol=1e-9))
    t.update(windows({"select_path": lambda: pl.select_path(J, max_rot_dev_allowed=allowed), "select": lambda: pl.select(J),
                      "over_the_host": lambda: over_the_host(eng, pl, r, hold, dt, obstacle, allowed)},
                     a.window, a.windows, lambda: pl.path_score(J, out={"invalid": np.zeros(p.B, dtype=np.int32)})))
    row = dict(case="wam", B=p.B, N=N, obs_check_inter=5, mode="orientation", link=LINK, sigma=SIGMA, constrained_states=N + 1,
               fixed_iterations=a.iters, inter_step=J, checked_states=N * (J + 1) + 1, best=new["best"],
               n_eligible=new["n_eligible"], solves_agree=solves_agree, check_agrees_with_host=check_agrees)
    print(f"workspace path on the headline WAM plan: B = {p.B}, N = {N}, ORIENTATION target on all {N + 1} states, "
          f"{a.windows} windows of {a.window} s, Gauss-Newton x{a.iters}")
    print(f"{'call':<22}{'median ms':>12}{'min ms':>12}{'max ms':>12}")
    for name, x in t.items():
        row[name + "_ms"] = dict(median=round(1e3 * statistics.median(x), 4), min=round(1e3 * min(x), 4), max=round(1e3 * max(x), 4))
        print(f"{name:<22}{1e3 * statistics.median(x):>12.4f}{1e3 * min(x):>12.4f}{1e3 * max(x):>12.4f}")
    med = lambda n: statistics.median(t[n])
    for kind in ("path", "factor"):
        row[f"{kind}_us_per_evaluation_pass"] = round(1e6 * (med("graph_error_" + kind) - med("graph_error_none")), 2)
        row[f"{kind}_us_per_solver_pass"] = round(1e6 * (med("solve_" + kind) - med("solve_none")) / (a.iters + 1), 2)
    print(f"per evaluation pass: fused path {row['path_us_per_evaluation_pass']} us, one workspace factor "
          f"{row['factor_us_per_evaluation_pass']} us; per solver pass: {row['path_us_per_solver_pass']} us against "
          f"{row['factor_us_per_solver_pass']} us")
    print(f"the two formulations solve alike: {solves_agree}; select_path agrees with the host computation: {check_agrees}")
    print(json.dumps(row), flush=True)
    for pl in plans.values():
        pl.close()
    return 0 if solves_agree and check_agrees else 1


if __name__ == "__main__":
    sys.exit(main())
