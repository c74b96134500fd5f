"""Cost of the moving-sphere factor per pass, and time of the moving check against the same answer over the host.

The workload is the headline WAM plan (restarts, B = 64, N = 100, obs_check_inter 5) created with room for 8 moving
spheres, so that it runs through the extras path in both variants: the resident set empty (K = 0: nothing is launched
for the factor) against K = 8 spheres that cross the arm's path (every pass then runs the sphere-centre kernel and
k_moving_accumulate).  Two clocks per variant: one evaluation pass (Plan.graph_error: the linearization, the factor, the
error reduction, B doubles back) and a Gauss-Newton run of --iters fixed iterations; the factor's cost per pass is the
difference of either pair.  The check: Plan.select_moving (inter_step 5) against get_result -> interpolate_traj ->
sphere_centers -> numpy distances, reduce, rule.

Per variant the median and min / max of the per-call time over --windows windows of >= --window seconds, variants
alternated, every shape warmed.  One JSON line; no ratio is asked for.

usage: python scripts/moving_throughput.py [--window 0.5] [--windows 5] [--iters 10] > profiles/moving_throughput.json"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, EPSILON, SIGMA, J = 8, 0.2, 0.01, 5


def crossing_spheres(eng, r, p):
    """K spheres that pass the straight-line trajectory's outer body spheres around mid-way, one after the other"""
    N, D, S = p.setting.total_step, p.setting.dof, r.S
    rng = np.random.default_rng(2)
    sk = rng.integers(S // 2, S, K)
    radius = rng.uniform(0.03, 0.08, K)
    u = rng.normal(size=(K, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    tm = rng.uniform(-0.4, 0.4, K)
    c, _ = eng.sphere_centers(r, p.init[0, N // 2, :D][None])
    t = np.linspace(-1.0, 1.0, N + 1)
    return radius, np.ascontiguousarray(c[0, sk][:, None, :] + u[:, None, :] * 1.2 * (t[None, :, None] - tm[:, None, None]))


def over_the_host(eng, pl, r, radius, centers, robot_radius, dt, obstacle, required):
    """the same pick through the entry points that existed before: two host round trips and a numpy reduce"""
    from gpmp2_amd import scoring
    from gpmp2_amd._capi import dptr
    res = pl.result()
    traj = res["traj"]
    B, D, N = traj.shape[0], r.dof, traj.shape[1] - 1
    up = eng.interpolate_traj(D, False, None, dt, J, traj)
    Md = up.shape[1]
    conf = np.ascontiguousarray(up[:, :, :D]).reshape(-1, D)
    c = np.zeros((conf.shape[0], r.S, 3))
    eng._ck(eng.lib.gpmp2mi_sphere_centers(r.ptr, conf.shape[0], dptr(conf), dptr(c), None))   # no Jacobians
    o = np.zeros((len(radius), Md, 3))
    for j in range(J + 1):
        tau = float(j) / float(J + 1)
        o[:, j:Md - 1:J + 1] = centers[:, :-1] if j == 0 else centers[:, :-1] + tau * (centers[:, 1:] - centers[:, :-1])
    o[:, -1] = centers[:, N]
    d = c.reshape(B, Md, r.S, 1, 3) - o.transpose(1, 0, 2)[None, :, None, :, :]
    dist = np.sqrt((d * d).sum(axis=4))
    clr = (dist - ((robot_radius[:, None] + radius[None, :]) + EPSILON)[None, None]).reshape(B, -1)
    valid = np.isfinite(dist).reshape(B, -1)
    mn = np.where(valid, clr, np.inf).min(axis=1)
    best, n = scoring.moving_rule(res["final_error"], res["status"], obstacle["min_clearance"], obstacle["out_of_range"],
                                  0.0, False, min_moving_clearance=mn, moving_invalid=(~valid).sum(axis=1),
                                  required_moving_clearance=required)
    return dict(best=best, n_eligible=n, min_moving_clearance=mn, dense_best=up[best] if best >= 0 else None)


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
    p.setting.set_moving_spheres(K, EPSILON, SIGMA)
    r, s = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    radius, centers = crossing_spheres(eng, r, p)
    robot_radius = np.asarray(p.model.flat()["sphere_radius"], dtype=np.float64)
    dt = p.setting.total_time / p.setting.total_step
    args = (p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
    plans = {}
    for name, k in (("K0", 0), ("K8", K)):
        pl = eng.plan(r, s, p.setting, p.B)
        pl.set_problem(*args)
        if k:
            pl.set_moving_spheres(radius, centers)
        plans[name] = pl

    def solve(pl):
        pl.set_problem(*args)
        pl.optimize()

    sync = lambda: plans["K8"].graph_error(p.init)
    t = windows({"graph_error_K0": lambda: plans["K0"].graph_error(p.init),
                 "graph_error_K8": lambda: plans["K8"].graph_error(p.init),
                 "solve_K0": lambda: solve(plans["K0"]), "solve_K8": lambda: solve(plans["K8"])}, a.window, a.windows, sync)
    # the check, on the K = 0 solution (rows that run through the spheres) given the spheres afterwards
    pl = plans["K0"]
    pl.set_moving_spheres(radius, centers)
    obstacle = pl.score(J)
    required = -0.1
    new = pl.select_moving(J, required)
    dev = pl.moving_score(J)
    old = over_the_host(eng, pl, r, radius, centers, robot_radius, dt, obstacle, required)
    agree = bool((new["best"], new["n_eligible"]) == (old["best"], old["n_eligible"]) and
                 np.allclose(dev["min_moving_clearance"], old["min_moving_clearance"], rtol=0, atol=1e-9))
    t.update(windows({"select_moving": lambda: pl.select_moving(J, required), "select": lambda: pl.select(J),
                      "over_the_host": lambda: over_the_host(eng, pl, r, radius, centers, robot_radius, dt, obstacle, required)},
                     a.window, a.windows, lambda: pl.moving_score(J, out={"invalid": np.zeros(p.B, dtype=np.int32)})))
    active = int((dev["min_moving_clearance"] < -EPSILON).sum())
    row = dict(case="wam", B=p.B, N=p.setting.total_step, obs_check_inter=5, spheres=r.S, moving_spheres=K, pairs=r.S * K,
               fixed_iterations=a.iters, inter_step=J, checked_states=p.setting.total_step * (J + 1) + 1,
               rows_in_contact=active, best=new["best"], n_eligible=new["n_eligible"], agrees_with_host=agree)
    for name, v in t.items():
        row[name + "_ms"] = dict(median=round(1e3 * statistics.median(v), 4), min=round(1e3 * min(v), 4),
                                 max=round(1e3 * max(v), 4))
    med = lambda n: statistics.median(t[n])
    row["factor_us_per_evaluation_pass"] = round(1e6 * (med("graph_error_K8") - med("graph_error_K0")), 2)
    row["factor_us_per_solver_pass"] = round(1e6 * (med("solve_K8") - med("solve_K0")) / (a.iters + 1), 2)
    print(json.dumps(row), flush=True)
    for pl in plans.values():
        pl.close()
    return 0 if agree else 1


if __name__ == "__main__":
    sys.exit(main())
