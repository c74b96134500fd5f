"""The measured table behind the bound of tests/test_gpu_posterior.py: every bounded case of that file (the stand-alone
chains, n = 1..15, and the plan-level cases), run `--runs` times on the GPU, with e_gpu, e_cpu (the larger of the two
float64 CPU values of the same system), their ratio and, for plans, e_gpu against the engine's own linearize; then the
K / FLOOR the rule gives.

    python scripts/posterior_error.py [--runs 2] > profiles/posterior_error.txt
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from gpmp2_amd import engine  # noqa: E402
from oracle import Oracle  # noqa: E402
import test_gpu_posterior as T  # noqa: E402


def one_run(eng, orc):
    rows = []
    for n in range(1, 16):
        rows += T.measure_chain(eng, n)
    for cid, make in T.PLAN_CASES:
        rows += T.measure_plan(eng, orc, cid, make)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=2)
    a = ap.parse_args()
    eng, orc = engine.Engine(), Oracle()
    runs = []
    for k in range(a.runs):
        runs.append(one_run(eng, orc))
        print(f"run {k}: {len(runs[-1])} rows", file=sys.stderr, flush=True)
    first = runs[0]
    print(f"# e = worst entry of the band on correlation scale (samples: sigma scale), worst trajectory "
          f"(tests/posterior_reference.py); {a.runs} runs")
    print(f"# {'case':42s} {'e_gpu':>9s} {'e_cpu':>9s} {'ratio':>8s} {'e_own':>9s}  same in every run")
    worst_ratio, floor_e, all_same = 0.0, 0.0, True
    for i, r in enumerate(first):
        same = all(o[i]["e_gpu"] == r["e_gpu"] for o in runs[1:])
        all_same &= same
        for o in runs:
            q = o[i]
            if q["e_cpu"] > 0:
                worst_ratio = max(worst_ratio, q["e_gpu"] / q["e_cpu"])
            if q["e_cpu"] < T.CPU_EXACT:
                floor_e = max(floor_e, q["e_gpu"])
        ratio = r["e_gpu"] / r["e_cpu"] if r["e_cpu"] > 0 else float("inf")
        own = f"{r['e_own']:9.2e}" if "e_own" in r else " " * 9
        print(f"  {r['id']:42s} {r['e_gpu']:9.2e} {r['e_cpu']:9.2e} {ratio:8.2f} {own}  {'yes' if same else 'NO'}")
    K = 2.0 ** math.ceil(math.log2(4.0 * worst_ratio)) if worst_ratio > 0 else float("nan")
    if K == 4.0 * worst_ratio:
        K *= 2.0
    print(f"# largest e_gpu / e_cpu {worst_ratio:.3f} -> K = next power of two above 4 x that = {K:g}")
    print(f"# largest e_gpu among the cases with e_cpu < {T.CPU_EXACT:g}: {floor_e:.3e} -> FLOOR = 4 x that = {4.0 * floor_e:.3e}")
    print(f"# hard cap {T.CAP:g} (a condition, not measured); in the test file now: K = {T.K:g}, FLOOR = {T.FLOOR:g}")
    print(f"# the {a.runs} runs gave {'identical values for every case' if all_same else 'DIFFERENT values for some cases (see the last column)'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
