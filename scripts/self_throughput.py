"""Time of the self-collision check with selection (Plan.select_checked) against the same answer over the host:
get_result -> interpolate_traj -> sphere_centers -> numpy pair distances, reduce, rule.  Two sizes: the headline problem
(WAM restarts, B = 64, N = 100, inter_step 5, the 78 generated pairs) and the PR2 model (dof 18, 65 spheres, N = 50,
inter_step 5) with its generated list.

Every size is measured in a process of its own, started here under a time limit; the first one that fails ends the run.
Per variant the median and min / max of the per-call time over --windows windows of >= --window seconds, variants
alternated, every shape warmed.  One JSON line per size; no ratio is asked for.

usage: python scripts/self_throughput.py [--window 0.5] [--windows 5] [--limit 240] > profiles/self_throughput.txt"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = ("wam", "pr2")


def pr2_problem(B):
    """the dof-18 PR2 problem of scripts/pr2_time.py (N = 50, I = 2, LM), B rows"""
    import gpmp2_amd as g
    from gpmp2_amd import problems
    from gpmp2_amd.settings import TrajOptimizerSetting
    model = g.generateMobileArm("PR2")
    origin, cell, data = problems.small3d_sdf(40)
    origin, cell, data = list(np.array(origin) * 3), cell * 3, data * 3
    D, N = 18, 50
    st = TrajOptimizerSetting(D)
    st.set_total_step(N); st.set_total_time(10.0); st.set_obs_check_inter(2); st.set_cost_sigma(0.1); st.set_epsilon(0.4)
    st.set_conf_prior_model(1e-3); st.set_vel_prior_model(1e-3); st.set_Qc_model(np.eye(D)); st.set_max_iter(30)
    st.setLM()
    start, end = np.zeros(D), np.zeros(D)
    start[:3] = [-1.5, -1.0, 0.3]; end[:3] = [1.5, 1.2, -0.4]; end[3] = 0.2
    end[4:] = np.tile(np.linspace(0.2, 0.8, 7), 2) * np.r_[np.ones(7), -np.ones(7)]
    rng = np.random.default_rng(3)
    init = np.zeros((B, N + 1, 2 * D))
    for b in range(B):
        amp = rng.normal(0, 0.1, size=D) * (b > 0)
        for i in range(N + 1):
            init[b, i, :D] = start * (N - i) / N + end * i / N + np.sin(np.pi * i / N) * amp
        init[b, :, D:] = (end - start)[None, :] / 10.0
    z = np.zeros((B, D))
    return problems.Problem("pr2", model, origin, cell, data, st, np.repeat(start[None], B, 0), z.copy(),
                            np.repeat(end[None], B, 0), z.copy(), init)


def over_the_host(eng, pl, r, lie, table, radius, dt, J, obstacle):
    """the same pick through the entry points that existed before: two host round trips and a numpy reduce"""
    from gpmp2_amd import scoring
    from gpmp2_amd._capi import dptr
    res = pl.result()
    traj = res["traj"]
    B, D = traj.shape[0], r.dof
    up = eng.interpolate_traj(D, lie, None, dt, J, traj)
    conf = np.ascontiguousarray(up[:, :, :D]).reshape(-1, D)
    centers = np.zeros((conf.shape[0], r.S, 3))
    eng._ck(eng.lib.gpmp2mi_sphere_centers(r.ptr, conf.shape[0], dptr(conf), dptr(centers), None))   # no Jacobians
    a, b = table[:, 0].astype(int), table[:, 1].astype(int)
    d = centers[:, a, :] - centers[:, b, :]
    dist = np.sqrt((d * d).sum(axis=2)).reshape(B, -1)
    clr = dist - np.tile(radius[a] + radius[b] + table[:, 2], up.shape[1])[None]
    valid = np.isfinite(dist)
    mn = np.where(valid, clr, np.inf).min(axis=1)
    best, n = scoring.select_rule(res["final_error"], res["status"], obstacle["min_clearance"], obstacle["out_of_range"], 0.0,
                                  False, mn, (~valid).sum(axis=1), 0.0)
    return dict(best=best, n_eligible=n, min_self_clearance=mn, dense_best=up[best] if best >= 0 else None)


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


def measure(case, window, count):
    from gpmp2_amd import engine, problems
    eng = engine.Engine()
    J = 5
    if case == "wam":
        p = problems.wam_restarts(B=64, total_step=100, obs_check_inter=5)
        gap = 2
    else:
        p = pr2_problem(16)
        gap = 2
    r, s = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pl = eng.plan(r, s, p.setting, p.B)
    pl.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
    pl.optimize()
    pairs = eng.generate_self_pairs(r, gap, np.zeros((1, r.dof)))
    dt = p.setting.total_time / p.setting.total_step
    lie = p.model.flat()["kind"] >= 2
    radius = np.asarray(p.model.flat()["sphere_radius"], dtype=np.float64)
    obstacle = pl.score(J)
    new = pl.select_checked(J, pairs)
    old = over_the_host(eng, pl, r, lie, pairs.data, radius, dt, J, obstacle)
    dev = pl.self_score(pairs, J)
    agree = bool((new["best"], new["n_eligible"]) == (old["best"], old["n_eligible"]) and
                 np.allclose(dev["min_self_clearance"], old["min_self_clearance"], rtol=0, atol=1e-9))
    t = windows({"select_checked": lambda: pl.select_checked(J, pairs),
                 "select": lambda: pl.select(J),
                 "over_the_host": lambda: over_the_host(eng, pl, r, lie, pairs.data, radius, dt, J, obstacle)},
                window, count, lambda: pl.self_score(pairs, J, out={"invalid": np.zeros(p.B, dtype=np.int32)}))
    row = dict(case=case, B=p.B, N=p.setting.total_step, inter_step=J, spheres=r.S, pairs=pairs.P,
               checked_states=p.setting.total_step * (J + 1) + 1, best=new["best"], n_eligible=new["n_eligible"],
               agrees_with_host=agree)
    for name, v in t.items():
        row[name + "_ms"] = dict(median=round(1e3 * statistics.median(v), 4), min=round(1e3 * min(v), 4),
                                 max=round(1e3 * max(v), 4))
    print(json.dumps(row), flush=True)
    pl.close()
    return 0 if agree else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds a size may take")
    ap.add_argument("--case", choices=CASES, help="measure this size in this process")
    a = ap.parse_args()
    if a.case:
        return measure(a.case, a.window, a.windows)
    for case in CASES:   # a process and a time limit per size; the first failure ends the run
        rc = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--case", case,
                             "--window", str(a.window), "--windows", str(a.windows)]).returncode
        if rc != 0:
            print(f"# {case}: exit status {rc}; stopped here", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
