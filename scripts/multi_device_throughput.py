"""Throughput of M WAM restarts (the headline graph: N = 100, I = 5, Synth200, Gauss-Newton) through a multi-device
plan (MultiPlan) for each --devices list, against one plain plan of the same B.  Two modes each: "queue" (one
optimize_queue call for all M problems) and "chunked" (set_problem / optimize / result per B problems, the last chunk
padded).  Every mode starts and ends on host arrays.  One JSON line per (B, devices, mode): traj/s (median of --reps
timed runs after one warm-up).
usage: python scripts/multi_device_throughput.py [--M 4096] [--B 64 256] [--devices 0 0,0] [--reps 3]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpmp2_amd import engine, problems  # noqa: E402


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def chunked(pl, rows, B):
    M = rows[0].shape[0]
    for c0 in range(0, M, B):
        idx = list(range(c0, min(c0 + B, M)))
        pad = idx + [idx[-1]] * (B - len(idx))
        pl.set_problem(*[a[pad] for a in rows])
        pl.optimize()
        pl.result()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=4096)
    ap.add_argument("--B", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--devices", nargs="+", default=["0", "0,0"], help="comma-separated device lists, one multi plan each")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    eng = engine.Engine()
    M = a.M
    p = problems.wam_restarts(B=M, opt="GN")
    rows = (p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
    r, s = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)

    def line(B, devices, mode, t):
        print(json.dumps(dict(M=M, B=B, devices=devices, mode=mode, traj_per_s=round(M / t), ms=round(1e3 * t, 3))),
              flush=True)

    for B in a.B:
        pl = eng.plan(r, s, p.setting, B)
        line(B, "plan", "queue", timed(lambda: pl.optimize_queue(*rows), a.reps))
        line(B, "plan", "chunked", timed(lambda: chunked(pl, rows, B), a.reps))
        pl.close()
        for spec in a.devices:
            devices = [int(x) for x in spec.split(",")]
            mp = eng.multi_plan(r, s, p.setting, B, devices)
            line(B, devices, "queue", timed(lambda: mp.optimize_queue(*rows), a.reps))
            line(B, devices, "chunked", timed(lambda: chunked(mp, rows, B), a.reps))
            mp.close()


if __name__ == "__main__":
    main()
