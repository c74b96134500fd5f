"""The measured table behind the bounds of tests/test_gpu_risk.py: every bounded case of that file (the stand-alone
covariance and risk calls on a float64 band, the random bands of dof 8 and 18, the plan-level cases), run `--runs` times
on the GPU, with e_gpu, e_cpu (the larger float64 CPU value of the same case), their ratio and, for plans, e_gpu against
the engine's own linearize; then the K / FLOOR the rule gives for each of the two measures.

    python scripts/risk_error.py [--runs 2] > profiles/risk_error.txt
"""
import argparse
import contextlib
import io
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from gpmp2_amd import engine  # noqa: E402
from oracle import Oracle  # noqa: E402
import test_gpu_risk as T  # noqa: E402


def one_run(eng, orc):
    rows = []
    with contextlib.redirect_stdout(io.StringIO()):       # the per-row prints of the comparisons
        for cid, make, J in T.CASES:
            rows += T.measure_standalone(eng, orc, cid, make, J)
        for dof in (8, 18):
            rows += T.measure_wide(eng, dof)
        for cid, make, J in T.CASES:
            rows += T.measure_plan(eng, orc, cid, make, J)
    return rows


def rule(rows_by_run, kind):
    worst_ratio, floor_e = 0.0, 0.0
    for o in rows_by_run:
        for q in o:
            if q["kind"] != kind:
                continue
            if q["e_cpu"] > 0:
                worst_ratio = max(worst_ratio, q["e_gpu"] / q["e_cpu"])
            if q["e_cpu"] < T.CPU_EXACT:
                floor_e = max(floor_e, q["e_gpu"])
    K = 2.0 ** math.ceil(math.log2(4.0 * worst_ratio)) if worst_ratio > 0 else float("nan")
    if K == 4.0 * worst_ratio:
        K *= 2.0
    return worst_ratio, K, floor_e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=2)
    a = ap.parse_args()
    eng, orc = engine.Engine(), Oracle()
    runs = []
    for k in range(a.runs):
        runs.append(one_run(eng, orc))
        print(f"run {k}: {len(runs[-1])} rows", file=sys.stderr, flush=True)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    print(f"# e_cov: worst entry of the dense blocks on correlation scale; e_sig: worst |sigma^^2 - sigma^2| / sbar^2 over the "
          f"in-range pairs; worst trajectory (tests/risk_reference.py); {a.runs} runs; on top of commit {commit or 'unknown'}")
    print("# rule: bound = min(max(K e_cpu, FLOOR), CAP) per measure; K = next power of two above 4 x the largest e_gpu / e_cpu,")
    print(f"#       FLOOR = 4 x the largest e_gpu among the cases with e_cpu < {T.CPU_EXACT:g}; CAP = {T.CAP:g} is a condition, not measured")
    print(f"# {'case':40s} {'':4s} {'e_gpu':>9s} {'e_cpu':>9s} {'ratio':>8s} {'e_own':>9s}  same in every run")
    all_same = True
    for i, r in enumerate(runs[0]):
        same = all(o[i]["e_gpu"] == r["e_gpu"] for o in runs[1:])
        all_same &= same
        ratio = r["e_gpu"] / r["e_cpu"] if r["e_cpu"] > 0 else float("inf")
        own = f"{r['e_own']:9.2e}" if "e_own" in r else " " * 9
        print(f"  {r['id']:40s} {r['kind']:4s} {r['e_gpu']:9.2e} {r['e_cpu']:9.2e} {ratio:8.2f} {own}  {'yes' if same else 'NO'}")
    for kind, Kt, Ft in (("cov", T.K_COV, T.FLOOR_COV), ("sig", T.K_SIG, T.FLOOR_SIG)):
        wr, K, fe = rule(runs, kind)
        print(f"# e_{kind}: largest e_gpu / e_cpu {wr:.3f} -> K = {K:g}; largest e_gpu among e_cpu < {T.CPU_EXACT:g}: {fe:.3e} -> "
              f"FLOOR = {4.0 * fe:.3e}; in the test file now: K = {Kt:g}, FLOOR = {Ft:.3e}")
    print(f"# the {a.runs} runs gave {'identical values for every case' if all_same else 'DIFFERENT values for some cases (see the last column)'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
