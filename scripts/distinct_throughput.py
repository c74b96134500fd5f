"""Time of the distinct alternatives of a solved batch (Plan.select_distinct_dev: score, rule, all-pairs distances,
grouping, one representative per mode, nothing leaves the device) against the same answer through what existed before:
result() to the host, chunked numpy pairwise distances, scoring.group_rule.  The headline problem (WAM restarts,
N = 100, inter_step 5) at B = 64 and 1 024, both metrics.

Every size is measured in a process of its own, started here under a time limit; the first one that fails ends the run.
Per variant the median and min / max of the per-call time over --windows windows of >= --window seconds, variants
alternated, every shape warmed.  One JSON line per (size, metric).  The two variants do not do quite the same work: the
baseline takes the obstacle scores from ONE Plan.score call made outside the timed loop, the new path scores the rows
again on every call.  That counts against the new path, so the acceptance below is on the safe side.  Acceptance: the new path's median is below the
baseline's minimum ("accepted").  kernel_share: the time of traj_distances_dev + group_rows_dev on the fetched result
(the pair kernel with the full matrix, and the rule) over the time of the whole call.

usage: python scripts/distinct_throughput.py [--window 0.5] [--windows 5] [--limit 300] > profiles/distinct_throughput.txt"""
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
SIZES = (64, 1024)
J, MAX_ALT = 5, 8


def host_distances(traj, D, metric):
    """float64 pairwise distances, a chunk of rows against all at a time: the [chunk][B][N+1][D] differences are kept
    near 4 096 pairs (23 MB at N = 100, D = 7) whatever B is"""
    x = np.ascontiguousarray(traj[:, :, :D])
    B = x.shape[0]
    chunk = max(1, 4096 // B)
    out = np.empty((B, B))
    for b0 in range(0, B, chunk):
        diff = x[b0:b0 + chunk, None] - x[None]
        s = np.einsum("abid,abid->abi", diff, diff)
        out[b0:b0 + chunk] = np.sqrt(s.max(axis=2) if metric == 0 else s.sum(axis=2) / x.shape[1])
    return out


def over_the_host(pl, D, metric, radius, scores):
    from gpmp2_amd import scoring
    res = pl.result()
    el = scoring.eligible(res["final_error"], res["status"], scores["min_clearance"], scores["out_of_range"], 0.0, False)
    dist = host_distances(res["traj"], D, metric)
    mode, leaders, sizes, n = scoring.group_rule(dist, res["final_error"], el, radius)
    k = min(n, MAX_ALT)
    return dict(n_modes=n, n_eligible=int(el.sum()), alt=leaders[:k], alt_size=sizes[:k], mode=mode, dist=dist)


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


def measure(B, window, count):
    import torch
    torch.cuda.init()
    from gpmp2_amd import engine, problems
    eng = engine.Engine()
    p = problems.wam_restarts(B=B, total_step=100, obs_check_inter=5)
    D, N = 7, p.setting.total_step
    r, s = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pl = eng.plan(r, s, p.setting, p.B)
    pl.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
    pl.optimize()
    scores = pl.score(J)
    Md = N * (J + 1) + 1
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    o = dict(n_modes=i32(1), n_eligible=i32(1), alt=i32(MAX_ALT), alt_size=i32(MAX_ALT), alt_error=f64(MAX_ALT),
             mode=i32(B), traj_alt=f64(MAX_ALT, N + 1, 2 * D), dense_alt=f64(MAX_ALT, Md, 2 * D))
    traj_d = torch.tensor(pl.result()["traj"], device="cuda")
    fe_d = torch.tensor(pl.result()["final_error"], device="cuda")
    dist_d, outs = f64(B, B), [i32(B), i32(B), i32(B), i32(1)]
    rc = 0
    for metric in (0, 1):
        # radius: the geometric mean of the two sides of the largest gap between the sorted distances of the result
        d = host_distances(pl.result()["traj"], D, metric)
        v = np.unique(d[np.triu_indices(B, 1)])
        v = v[np.isfinite(v) & (v > 0)]
        g = int(np.argmax(np.diff(v)))
        radius = float(np.sqrt(v[g] * v[g + 1]))
        new = pl.select_distinct(J, radius, MAX_ALT, 0.0, False, metric=metric)
        old = over_the_host(pl, D, metric, radius, scores)
        k = min(new["n_modes"], MAX_ALT)
        agree = bool(new["n_modes"] == old["n_modes"] and new["n_eligible"] == old["n_eligible"] and
                     np.array_equal(new["alt"][:k], old["alt"]) and np.array_equal(new["alt_size"][:k], old["alt_size"]) and
                     np.array_equal(new["mode"], old["mode"]))
        t = windows({"select_distinct_dev": lambda: pl.select_distinct_dev(J, radius, MAX_ALT, 0.0, False, metric=metric, **o),
                     "select_dev": lambda: pl.select_dev(J),
                     "pairs_and_rule": lambda: (eng.traj_distances_dev(D, B, N, traj_d, dist_d, None, metric),
                                                eng.group_rows_dev(B, dist_d, fe_d, None, radius, *outs)),
                     "over_the_host": lambda: over_the_host(pl, D, metric, radius, scores)},
                    window, count, torch.cuda.synchronize)
        row = dict(B=B, N=N, inter_step=J, metric=("max_state", "rms")[metric], radius=radius, n_modes=new["n_modes"],
                   n_eligible=new["n_eligible"], sizes=[int(x) for x in new["alt_size"][:k]], agrees_with_host=agree)
        for name, x in t.items():
            row[name + "_ms"] = dict(median=round(1e3 * statistics.median(x), 4), min=round(1e3 * min(x), 4),
                                     max=round(1e3 * max(x), 4))
        row["kernel_share"] = round(row["pairs_and_rule_ms"]["median"] / row["select_distinct_dev_ms"]["median"], 3)
        row["accepted"] = bool(row["select_distinct_dev_ms"]["median"] < row["over_the_host_ms"]["min"])
        print(json.dumps(row), flush=True)
        rc |= 0 if agree else 1
    pl.close()
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds a size may take")
    ap.add_argument("--size", type=int, choices=SIZES, help="measure this size in this process")
    a = ap.parse_args()
    if a.size:
        return measure(a.size, a.window, a.windows)
    for B in SIZES:   # a process and a time limit per size; the first failure ends the run
        rc = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--size", str(B),
                             "--window", str(a.window), "--windows", str(a.windows)]).returncode
        if rc != 0:
            print(f"# B={B}: exit status {rc}; stopped here", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
