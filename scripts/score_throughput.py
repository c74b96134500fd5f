"""Time of "plan, then pick": the score-and-select stage (Plan.select_dev / Plan.select) on the headline problem (WAM
restarts, N = 100, I = 5, Synth200, Gauss-Newton, after optimize) against what the same answers cost through the entry
points that existed before it: get_result -> interpolate_traj -> collision_cost on the up-sampled rows ->
sphere_centers + sdf_query for the clearance -> numpy reduce and argmin.

Same process, variants alternated, every shape warmed; a window is >= --window seconds of repeated calls ended by a device
synchronise; per variant the median and min / max of the per-call time over --windows windows.  One JSON line.
`accept`: the new path's median is below the baseline's minimum.  Algorithmic bytes of the scoring kernel per row:
Md * S * 8 corners * 8 B.

usage: python scripts/score_throughput.py [--B 1 64 1024] [--inter 5 9] [--window 0.5] [--windows 5]
       python scripts/score_throughput.py --trace     (a short run for rocprofv3 --kernel-trace --stats: no timing)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch                      # torch's HIP runtime first, as bench.py does; it owns the device outputs

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpmp2_amd import engine, problems, scoring  # noqa: E402
from gpmp2_amd._capi import dptr, iptr  # noqa: E402


def baseline(eng, pl, r, s, radius, dt, J):
    """the same answers through the older entry points: four host round trips and a numpy reduce"""
    res = pl.result()
    traj = res["traj"]
    B, N, D, S = traj.shape[0], traj.shape[1] - 1, r.dof, r.S
    up = eng.interpolate_traj(D, False, None, dt, J, traj)
    Md = up.shape[1]
    support = eng.collision_cost(r, s, N, traj)
    dense = eng.collision_cost(r, s, Md - 1, up)
    conf = np.ascontiguousarray(up[:, :, :D]).reshape(-1, D)
    centers = np.zeros((conf.shape[0], S, 3))
    eng._ck(eng.lib.gpmp2mi_sphere_centers(r.ptr, conf.shape[0], dptr(conf), dptr(centers), None))
    M = conf.shape[0] * S
    dist, inr = np.zeros(M), np.zeros(M, dtype=np.int32)
    eng._ck(eng.lib.gpmp2mi_sdf_query(s.ptr, M, dptr(centers.reshape(M, 3)), dptr(dist), None, iptr(inr)))
    inr = inr.reshape(B, Md, S).astype(bool)
    clr = np.where(inr, dist.reshape(B, Md, S) - radius, np.inf).reshape(B, Md * S)
    arg = clr.argmin(axis=1)
    mn, oor = clr[np.arange(B), arg], (~inr).reshape(B, Md * S).sum(axis=1)
    best, n = scoring.select_rule(res["final_error"], res["status"], mn, oor, 0.0, True)
    return dict(best=best, n_eligible=n, support_cost=support, dense_cost=dense, min_clearance=mn, worst=arg,
                traj_best=traj[best] if best >= 0 else None, dense_best=up[best] if best >= 0 else None)


def windows(variants, window, count):
    """alternates the variants; per variant the per-call seconds of `count` windows"""
    out = {name: [] for name in variants}
    for name, fn in variants.items():    # warm every shape
        fn()
    torch.cuda.synchronize()
    for _ in range(count):
        for name, fn in variants.items():
            calls, t0 = 0, time.perf_counter()
            while True:
                fn()
                calls += 1
                if time.perf_counter() - t0 >= window:
                    break
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t0) / calls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--inter", type=int, nargs="+", default=[5, 9])
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    torch.cuda.init()
    eng = engine.Engine()
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    cases = []
    for B in ([64] if a.trace else a.B):
        p = problems.wam_restarts(B=B, opt="GN")
        r, s = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
        N, D, S = p.setting.total_step, p.setting.dof, r.S
        dt = p.setting.total_time / N
        radius = np.asarray(p.model.flat()["sphere_radius"], dtype=np.float64).reshape(1, 1, S)
        pl = eng.plan(r, s, p.setting, B)
        pl.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
        pl.optimize()
        for J in ([5] if a.trace else a.inter):
            Md = scoring.checked_states(N, J)
            best = torch.zeros(1, dtype=torch.int32, device=dev)
            n = torch.zeros(1, dtype=torch.int32, device=dev)
            tb = torch.zeros((N + 1, 2 * D), dtype=torch.float64, device=dev)
            db = torch.zeros((Md, 2 * D), dtype=torch.float64, device=dev)

            def new_dev():
                pl.select_dev(J, 0.0, True, best=best, n_eligible=n, traj_best=tb, dense_best=db, stream=st.cuda_stream)
                st.synchronize()

            def new_host():
                return pl.select(J, 0.0, True)

            if a.trace:
                pl.optimize()
                for _ in range(20):
                    new_dev()
                continue
            # the three variants give the same answers
            ref, got = baseline(eng, pl, r, s, radius, dt, J), new_host()
            new_dev()
            sc = pl.score(J)
            assert got["best"] == ref["best"] == int(best.cpu()[0]) and got["n_eligible"] == ref["n_eligible"], (got["best"], ref["best"])
            np.testing.assert_allclose(sc["dense_cost"], ref["dense_cost"], rtol=1e-8, atol=1e-12)
            np.testing.assert_allclose(sc["min_clearance"], ref["min_clearance"], rtol=0, atol=1e-9)
            if ref["best"] >= 0:
                assert np.array_equal(got["dense_best"], ref["dense_best"]) and np.array_equal(db.cpu().numpy(), ref["dense_best"])
            t = windows({"baseline": lambda: baseline(eng, pl, r, s, radius, dt, J), "select_dev": new_dev,
                         "select_host": new_host}, a.window, a.windows)
            row = dict(B=B, N=N, inter_step=J, checked_states=Md, spheres=S, best=ref["best"], n_eligible=ref["n_eligible"],
                       algorithmic_bytes=B * Md * S * 64)
            for name, ts in t.items():
                row[name + "_ms"] = dict(median=round(1e3 * statistics.median(ts), 4), min=round(1e3 * min(ts), 4),
                                         max=round(1e3 * max(ts), 4), windows=len(ts))
            row["accept"] = bool(row["select_dev_ms"]["median"] < row["baseline_ms"]["min"]
                                 and row["select_host_ms"]["median"] < row["baseline_ms"]["min"])
            cases.append(row)
        pl.close()
    if not a.trace:
        print(json.dumps(dict(script="score_throughput", problem="wam_restarts N=100 I=5 Synth200 GN", window_s=a.window,
                              cases=cases)))


if __name__ == "__main__":
    main()
