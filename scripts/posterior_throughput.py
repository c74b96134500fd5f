"""Time of the posterior of a solved plan on the headline problem (WAM restarts, N = 100, I = 5, Synth200, Gauss-Newton,
after optimize): Plan.marginals_dev and Plan.sample_posterior_dev (K = 16) against the only way to the same answers
before them: Plan.linearize to the host, then the float64 block recursion of tests/posterior_reference.py per trajectory.

Same process, variants alternated, every shape warmed; a window is >= --window seconds of repeated calls ended by a
device synchronise; per variant the median and min / max of the per-call time over --windows windows.  The baseline's
recursion is interpreted Python (tens of milliseconds per trajectory): it is timed over the first --base-rows
trajectories and scaled to B, its linearize over all B; one call per window.  One JSON line.

usage: python scripts/posterior_throughput.py [--B 64 1024] [--K 16] [--window 0.5] [--windows 5] [--base-rows 16]
       python scripts/posterior_throughput.py --trace     (a short run for rocprofv3 --kernel-trace --stats: no timing)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch                      # torch's HIP runtime first, as bench.py does; it owns the device outputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from gpmp2_amd import engine, problems  # noqa: E402
import posterior_reference as ref  # noqa: E402


def windows(variants, window, count):
    """alternates the variants; per variant the per-call seconds of `count` windows"""
    out = {name: [] for name in variants}
    for fn in variants.values():    # warm every shape
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
    ap.add_argument("--B", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--K", type=int, default=16)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--base-rows", type=int, default=16)
    ap.add_argument("--base-windows", type=int, default=3)
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
        N, D, K = p.setting.total_step, p.setting.dof, a.K
        nb, n = N + 1, 2 * D
        pl = eng.plan(r, s, p.setting, B)
        pl.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
        pl.optimize()
        traj = pl.result()["traj"]
        Sd = torch.zeros((B, nb, n, n), dtype=torch.float64, device=dev)
        So = torch.zeros((B, nb - 1, n, n), dtype=torch.float64, device=dev)
        ok = torch.zeros((B,), dtype=torch.int32, device=dev)
        z = torch.randn((B, K, nb, n), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        dl = torch.zeros_like(z)

        def marginals_dev():
            pl.marginals_dev(Sd, So, ok, stream=st.cuda_stream)
            st.synchronize()

        def sample_dev():
            pl.sample_posterior_dev(K, z, dl, stream=st.cuda_stream)
            st.synchronize()

        if a.trace:
            for _ in range(20):
                marginals_dev()
                sample_dev()
            pl.close()
            continue
        rows = min(B, a.base_rows)
        base = dict(linearize=[], recursion=[], sample=[])
        host = None
        for _ in range(a.base_windows):
            t0 = time.perf_counter()
            Hd, Ho, _, _ = pl.linearize(traj)
            t1 = time.perf_counter()
            host = [ref.marginals(Hd[b], Ho[b]) for b in range(rows)]
            t2 = time.perf_counter()
            zh = np.zeros((K, nb, n))
            for b in range(rows):
                ref.sample(Hd[b], Ho[b], zh)
            t3 = time.perf_counter()
            base["linearize"].append(t1 - t0)
            base["recursion"].append((t2 - t1) * B / rows)
            base["sample"].append((t3 - t2) * B / rows)
        # the answers agree (correlation scale, against the float64 recursion of the same exported system)
        marginals_dev()
        got_d, got_o = Sd.cpu().numpy(), So.cpu().numpy()
        assert int(ok.sum()) == B
        agree = max(ref.cov_error(got_d[b], got_o[b], *host[b]) for b in range(rows))
        assert agree < 1e-9, agree
        t = windows({"marginals_dev": marginals_dev, "sample_dev": sample_dev}, a.window, a.windows)
        row = dict(B=B, N=N, dof=D, K=K, unknowns=nb * n, agreement=float(f"{agree:.3g}"),
                   marginals_dev_ms=stats(t["marginals_dev"]), sample_dev_ms=stats(t["sample_dev"]),
                   baseline_linearize_ms=stats(base["linearize"]), baseline_rows_timed=rows,
                   baseline_marginals_ms=stats([x + y for x, y in zip(base["linearize"], base["recursion"])]),
                   baseline_sample_ms=stats([x + y for x, y in zip(base["linearize"], base["sample"])]))
        row["marginals_speedup"] = round(row["baseline_marginals_ms"]["median"] / row["marginals_dev_ms"]["median"], 1)
        row["sample_speedup"] = round(row["baseline_sample_ms"]["median"] / row["sample_dev_ms"]["median"], 1)
        # against the transfer alone: what any host-side inverse pays before it starts
        row["marginals_vs_linearize_alone"] = round(row["baseline_linearize_ms"]["median"] / row["marginals_dev_ms"]["median"], 1)
        cases.append(row)
        pl.close()
    if not a.trace:
        print(json.dumps(dict(script="posterior_throughput", problem="wam_restarts N=100 I=5 Synth200 GN",
                              window_s=a.window, cases=cases)))


if __name__ == "__main__":
    main()
