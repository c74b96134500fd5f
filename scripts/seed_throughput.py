"""What seeding on the device buys on the headline problem (WAM restarts, N = 100, I = 5, Synth200, Gauss-Newton, a plan of
B = 64 slots):

  queue      M restarts through the plan.  baseline: the inits as numpy arrays + Plan.optimize_queue with host pointers
             (the path before seeding: M (N+1) 2D doubles cross to the device); new: Plan.optimize_queue_seeded (only the
             end configurations cross).  Both solve the SAME problems: the baseline's inits are the seeded ones, fetched
             once outside the timing, so the two differ in where the inits come from and in nothing else.
  posterior  K samples per row of the solved plan, device buffers.  baseline: Engine.normal_fill_dev + Plan.
             sample_posterior_dev (z through memory, one wavefront per row walks its K / 16 tiles in turn); new:
             Plan.sample_posterior_seeded_dev (z in registers, one wavefront per (tile, row)).

Same process, variants alternated, every shape warmed; a window is >= --window seconds of repeated calls ended by a device
synchronise; per variant the median and min / max of the per-call time over --windows windows.  One JSON line.
`accept`: the new path's median is below the baseline's minimum.

usage: python scripts/seed_throughput.py [--M 64 1024 4096] [--K 16 256 1024] [--window 0.5] [--windows 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch                      # torch's HIP runtime first, as bench.py does; it owns the device buffers

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpmp2_amd import _capi, engine, problems  # noqa: E402

SEED = 2026


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


def stats(ts):
    return dict(median=round(1e3 * statistics.median(ts), 4), min=round(1e3 * min(ts), 4), max=round(1e3 * max(ts), 4),
                windows=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, nargs="+", default=[64, 1024, 4096])
    ap.add_argument("--K", type=int, nargs="+", default=[16, 256, 1024])
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    torch.cuda.init()
    eng = engine.Engine()
    dev = torch.device("cuda:0")
    B = a.B
    p = problems.wam_restarts(B=B, opt="GN")
    r, s = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    N, D = p.setting.total_step, p.setting.dof
    pl = eng.plan(r, s, p.setting, B)
    queue, post = [], []
    for M in a.M:
        sc, ec = np.repeat(p.start_conf[:1], M, 0), np.repeat(p.end_conf[:1], M, 0)
        zv = np.zeros((M, D))
        kw = dict(scale=a.scale, keep_first=True)
        init = pl.seed_restarts(M, SEED, sc, ec, **kw)
        ref, got = pl.optimize_queue(sc, zv, ec, zv, init), pl.optimize_queue_seeded(SEED, sc, zv, ec, zv, **kw)
        assert all(np.array_equal(ref[k], got[k], equal_nan=k == "error_trace") for k in ref), "the two variants must give the same rows"
        t = windows({"baseline": lambda: pl.optimize_queue(sc, zv, ec, zv, init),
                     "seeded": lambda: pl.optimize_queue_seeded(SEED, sc, zv, ec, zv, **kw)}, a.window, a.windows)
        row = dict(M=M, B=B, N=N, init_bytes=int(init.nbytes), converged=int((ref["status"] == 0).sum()),
                   mean_iters=round(float(ref["iters"].mean()), 2), baseline_ms=stats(t["baseline"]),
                   seeded_ms=stats(t["seeded"]))
        row["accept"] = bool(row["seeded_ms"]["median"] < row["baseline_ms"]["min"])
        queue.append(row)
    pl.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
    pl.optimize()
    st = torch.cuda.Stream(device=dev)
    for K in a.K:
        shape = (B, K, N + 1, 2 * D)
        z = torch.zeros(shape, dtype=torch.float64, device=dev)
        d0, d1 = torch.zeros_like(z), torch.zeros_like(z)

        def base():
            eng.normal_fill_dev(SEED, _capi.RNG_POSTERIOR, 0, B, 0, K, N + 1, 2 * D, z, stream=st.cuda_stream)
            pl.sample_posterior_dev(K, z, d0, stream=st.cuda_stream)
            st.synchronize()

        def new():
            pl.sample_posterior_seeded_dev(K, SEED, d1, stream=st.cuda_stream)
            st.synchronize()

        base()
        new()
        worst = float((d0 - d1).abs().max().cpu())
        t = windows({"baseline": base, "seeded": new}, a.window, a.windows)
        row = dict(K=K, B=B, N=N, z_bytes=int(z.numel() * 8), max_abs_difference=worst, baseline_ms=stats(t["baseline"]),
                   seeded_ms=stats(t["seeded"]))
        row["accept"] = bool(row["seeded_ms"]["median"] < row["baseline_ms"]["min"])
        post.append(row)
        del z, d0, d1
    pl.close()
    print(json.dumps(dict(script="seed_throughput", problem="wam_restarts N=100 I=5 Synth200 GN", window_s=a.window,
                          queue=queue, posterior=post)))


if __name__ == "__main__":
    main()
