"""Throughput of a queue of WAM restarts (the headline graph: N = 100, I = 5, Synth200, Gauss-Newton) through one plan
(Plan.optimize_queue) against the chunked loop of set_problem / optimize / result on the same plan, and against one
plan of B = M.  Every mode starts and ends on host arrays.  One JSON line per (M, B, mode): traj/s (median of --reps
timed runs after one warm-up), passes and the busy fraction (slot-passes that held a problem / B * passes).
usage: python scripts/queue_throughput.py [--M 1024 4096] [--B 64 128 256 512] [--one-plan-max 4096] [--reps 3]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpmp2_amd import engine, problems  # noqa: E402


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def chunked(pl, rows):
    B, M = pl.B, rows[0].shape[0]
    passes = busy = 0
    for c0 in range(0, M, B):
        idx = list(range(c0, min(c0 + B, M)))
        pad = idx + [idx[-1]] * (B - len(idx))
        pl.set_problem(*[a[pad] for a in rows])
        pl.optimize()
        it = pl.result()["iters"]
        passes += int(it.max()) + 1
        busy += int((it[:len(idx)] + 1).sum())
    return passes, busy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--B", type=int, nargs="+", default=[64, 128, 256, 512])
    ap.add_argument("--one-plan-max", type=int, default=4096, help="largest M also run as one plan of B = M")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    eng = engine.Engine()
    for M in a.M:
        p = problems.wam_restarts(B=M, opt="GN")
        rows = (p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
        r, s = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)

        def line(B, mode, t, passes, busy):
            print(json.dumps(dict(M=M, B=B, mode=mode, traj_per_s=round(M / t), ms=round(1e3 * t, 3), passes=passes,
                                  busy_fraction=round(busy / (B * passes), 4))), flush=True)

        for B in a.B:
            pl = eng.plan(r, s, p.setting, B)
            t, _ = timed(lambda: pl.optimize_queue(*rows), a.reps)
            st = pl.queue_stats()
            line(B, "queue", t, st["passes"], st["busy_slot_passes"])
            t, (passes, busy) = timed(lambda: chunked(pl, rows), a.reps)
            line(B, "chunked", t, passes, busy)
            pl.close()
        if M <= a.one_plan_max:
            pl = eng.plan(r, s, p.setting, M)
            t, (passes, busy) = timed(lambda: chunked(pl, rows), a.reps)
            line(M, "one_plan", t, passes, busy)
            pl.close()


if __name__ == "__main__":
    main()
