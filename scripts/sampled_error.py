"""The measured table behind the bounds of tests/test_gpu_sampled.py: every bounded case of that file (the stand-alone
calls of three robots at six (N, J) and of three more planar arms, with and without the bridge, the plan-level cases), run `--runs` times on the GPU,
with e_gpu, e_cpu (the float64 spread of the same case) and their ratio; then the K_f / FLOOR the rule gives for each of
the two maps.  The count checks of the test file are run with the constants it holds now and reported, not asserted.

    python scripts/sampled_error.py [--runs 2] [--commit HASH] > profiles/sampled_error.txt
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
import sampled_cases as cases  # noqa: E402
import test_gpu_sampled as T  # noqa: E402

PLANS = (("wam", 5, 5), ("planar", 5, 5))


def one_run(eng, orc):
    rows, later = [], []
    with contextlib.redirect_stdout(io.StringIO()):
        for robot, N, J in cases.ALL:
            r, l = T.measure_standalone(eng, orc, robot, N, J)
            rows += r
            later += l
        for robot, N, J in PLANS:
            r, l = T.measure_plan(eng, orc, robot, N, J)
            rows += r
            later += l
    return rows, later


def rule(rows_by_run, kind):
    worst_ratio, floor_e = 0.0, 0.0
    for o in rows_by_run:
        for q in o:
            if q["kind"] != kind:
                continue
            if q["e_cpu"] >= T.RESOLVED:
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
    ap.add_argument("--commit", default="", help="the commit the tree stands on, where the run has no git history to ask")
    a = ap.parse_args()
    eng, orc = engine.Engine(), Oracle()
    runs, later = [], None
    for k in range(a.runs):
        rows, later = one_run(eng, orc)
        runs.append(rows)
        print(f"run {k}: {len(rows)} rows", file=sys.stderr, flush=True)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    commit = commit or a.commit
    print(f"# e_conf: max |conf - ref|; e_clr: max |state_clearance - ref| over the finite entries; the row with the largest "
          f"ratio (tests/sampled_reference.py); {a.runs} runs; on top of commit {commit or 'unknown'}")
    print("# rule: bound = min(max(K_f e_cpu, FLOOR), CAP) per map; K_f = next power of two above 4 x the largest e_gpu / e_cpu")
    print(f"#       among the cases whose e_cpu is resolved (>= 2^-52 = {T.RESOLVED:.2e}, one ulp of unity; ratios below are marked -),")
    print(f"#       FLOOR = 4 x the largest e_gpu among the cases with e_cpu < {T.CPU_EXACT:g}; CAP = {T.CAP:g} is a condition, not measured")
    print(f"# {'case':40s} {'':4s} {'e_gpu':>9s} {'e_cpu':>9s} {'ratio':>8s}  same in every run")
    all_same = True
    for i, r in enumerate(runs[0]):
        same = all(o[i]["e_gpu"] == r["e_gpu"] for o in runs[1:])
        all_same &= same
        ratio = f"{r['e_gpu'] / r['e_cpu']:8.2f}" if r["e_cpu"] >= T.RESOLVED else f"{'-':>8s}"
        print(f"  {r['id']:40s} {r['kind']:4s} {r['e_gpu']:9.2e} {r['e_cpu']:9.2e} {ratio}  {'yes' if same else 'NO'}")
    for kind, Kt, Ft in (("conf", T.K_CONF, T.FLOOR_CONF), ("clr", T.K_CLR, T.FLOOR_CLR)):
        wr, K, fe = rule(runs, kind)
        print(f"# e_{kind}: largest e_gpu / e_cpu {wr:.3f} -> K_f = {K:g}; largest e_gpu among e_cpu < {T.CPU_EXACT:g}: {fe:.3e} -> "
              f"FLOOR = {4.0 * fe:.3e}; in the test file now: K_f = {Kt:g}, FLOOR = {Ft:.3e}")
    print(f"# the {a.runs} runs gave {'identical values for every case' if all_same else 'DIFFERENT values for some cases (see the last column)'}")
    try:
        T.check_counts(later)
        print(f"# counts: all {len(later)} calls lie within the brackets of the constants the test file holds now")
    except AssertionError as e:
        print(f"# counts: FAILED with the constants the test file holds now: {e}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
