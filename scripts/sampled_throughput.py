"""Time of the sampled clearance of a solved plan (include/gpmp2mi.h "sampled clearance"): Plan.collision_probability_dev
(counts only, no maps) against Plan.sample_posterior_seeded_dev for the same K -- the part both share: linearize, export,
the factor sweep and the back-substitution -- so that their difference is the time of k_sampled_clearance and
k_sampled_finish.  WAM restarts, N = 100, Gauss-Newton, after optimize; --sdf names the field.

One library build per process: GPMP2MI_LIB selects a build with another SAMPLED_PER_WG, --label names it in the line.
Such a build is the product build with one macro more (everything is recompiled, launch.h holds the constant):
    make -C gpmp2_amd/csrc clean
    make -C gpmp2_amd/csrc -j16 EXTRA=-DG2_SAMPLED_PER_WG=4 OUT=../../build/spw4/libgpmp2mi.so     (mkdir -p build/spw4 first)
then `make clean` again and the plain build.  Same process, variants alternated,
every shape warmed; a window is >= --window seconds of repeated calls ended by a device synchronise; per variant the
median and min / max of the per-call time over --windows windows.  One JSON line.

usage: python scripts/sampled_throughput.py [--label 8] [--B 8] [--J 5] [--K 256 4096] [--sdf 40] [--window 0.3] [--windows 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch                      # torch's HIP runtime first, as bench.py does; it owns the device outputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from gpmp2_amd import engine, problems  # noqa: E402


def windows(variants, window, count):
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
    ap.add_argument("--label", default="8")
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--J", type=int, default=5)
    ap.add_argument("--K", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--sdf", default="40")
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    torch.cuda.init()
    eng = engine.Engine()
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    p = problems.wam_restarts(B=a.B, opt="GN", sdf=a.sdf)
    r, s = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    N, D, B, J = p.setting.total_step, p.setting.dof, a.B, a.J
    pl = eng.plan(r, s, p.setting, B)
    pl.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
    pl.optimize()
    cases = []
    for K in a.K:
        hits = torch.zeros((B,), dtype=torch.int32, device=dev)
        prob = torch.zeros((B,), dtype=torch.float64, device=dev)
        delta = torch.zeros((B, K, N + 1, 2 * D), dtype=torch.float64, device=dev)

        def probability():
            pl.collision_probability_dev(J, K, 7, 0.05, hits=hits, probability=prob, stream=st.cuda_stream)
            st.synchronize()

        def samples():
            pl.sample_posterior_seeded_dev(K, 7, delta, stream=st.cuda_stream)
            st.synchronize()

        t = windows({"probability": probability, "samples": samples}, a.window, a.windows)
        row = dict(K=K, collision_probability_dev_ms=stats(t["probability"]), sample_posterior_seeded_dev_ms=stats(t["samples"]),
                   hits=[int(x) for x in hits.cpu().numpy()])
        row["difference_ms"] = round(row["collision_probability_dev_ms"]["median"] - row["sample_posterior_seeded_dev_ms"]["median"], 4)
        row["samples_checked_per_s"] = round(B * K / (1e-3 * row["collision_probability_dev_ms"]["median"]))
        cases.append(row)
    pl.close()
    print(json.dumps(dict(script="sampled_throughput", samples_per_workgroup=a.label, library=os.path.relpath(engine.LIB_PATH, ROOT),
                          problem=f"wam_restarts N={N} I=5 sdf={a.sdf} GN", B=B, J=J, checked_states=N * (J + 1) + 1,
                          window_s=a.window, cases=cases)))


if __name__ == "__main__":
    main()
