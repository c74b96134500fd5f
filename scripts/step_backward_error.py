"""The measured table behind the bound of tests/test_gpu_step_backward_error.py: every case of that file, run `--runs`
times on the GPU, with eta_gpu (against the oracle's linearization), the same step against the engine's own linearize,
eta_oracle and their ratio, and the K / U_FLOOR the rule gives.

    python scripts/step_backward_error.py [--runs 2] [--lib other/libgpmp2mi.so] > profiles/step_backward_error.txt

A case whose own assertions fail (wrong kernel launched, no accepted step) is listed with the message and the run goes
on; an error of the library itself ends the run there."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from gpmp2_amd import engine  # noqa: E402
from oracle import Oracle  # noqa: E402
import test_gpu_step_backward_error as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--lib", default=engine.LIB_PATH)
    a = ap.parse_args()
    eng, orc = engine.Engine(a.lib), Oracle()
    cases = T.all_cases()
    runs, failed = [], []
    for k in range(a.runs):
        rows = {}
        for c in cases:
            try:
                rows[c.id] = m = T.measure(eng, orc, c)
                print(f"run {k} {c.id}: eta_gpu {m['eta_gpu']:.2e} eta_own {m['eta_own']:.2e} eta_oracle "
                      f"{m['eta_oracle']:.2e}", file=sys.stderr, flush=True)
            except (AssertionError, engine.Gpmp2miError) as e:
                if isinstance(e, engine.Gpmp2miError) and e.code != 4:   # 4: refused before anything was launched
                    raise
                rows[c.id] = None
                print(f"run {k} {c.id}: {e}", file=sys.stderr, flush=True)
                if k == 0:
                    failed.append((c.id, str(e).splitlines()[0][:160] if str(e) else repr(e)))
        runs.append(rows)
    first = runs[0]
    print(f"# one optimizer step per case; eta = worst block row, worst trajectory (tests/backward_error.py); {a.runs} runs")
    print(f"# {'case':45s} {'B':>3s} {'N':>4s} {'dof':>3s} {'eta_gpu':>9s} {'eta_own':>9s} {'eta_oracle':>10s} {'ratio':>7s}  same in every run")
    worst_ratio, worst_eta = 0.0, 0.0
    all_same = True
    for c in cases:
        m = first[c.id]
        if m is None:
            continue
        ratio = m["eta_gpu"] / m["eta_oracle"]
        worst_ratio, worst_eta = max(worst_ratio, ratio), max(worst_eta, m["eta_gpu"])
        same = all(r[c.id] is not None and r[c.id]["eta_gpu"] == m["eta_gpu"] and r[c.id]["eta_own"] == m["eta_own"]
                   for r in runs[1:])
        for r in runs[1:]:
            if r[c.id] is not None:
                worst_ratio = max(worst_ratio, r[c.id]["eta_gpu"] / r[c.id]["eta_oracle"])
                worst_eta = max(worst_eta, r[c.id]["eta_gpu"])
        all_same &= same
        print(f"  {c.id:45s} {m['B']:3d} {m['N']:4d} {m['dof']:3d} {m['eta_gpu']:9.2e} {m['eta_own']:9.2e} "
              f"{m['eta_oracle']:10.2e} {ratio:7.2f}  {'yes' if same else 'NO'}")
    for cid, msg in failed:
        print(f"  {cid:45s} FAILED ITS OWN ASSERTIONS: {msg}")
    K = 2.0 ** math.ceil(math.log2(4.0 * worst_ratio)) if worst_ratio > 0 else float("nan")
    if K == 4.0 * worst_ratio:
        K *= 2.0
    print(f"# largest eta_gpu / eta_oracle {worst_ratio:.3f} -> K = next power of two above 4 x that = {K:g}")
    print(f"# largest eta_gpu {worst_eta:.3e} -> U_FLOOR = 4 x that = {4.0 * worst_eta:.3e}")
    print(f"# hard cap {T.CAP:g} (a condition, not measured); in the test file now: K = {T.K:g}, U_FLOOR = {T.U_FLOOR:g}")
    print(f"# the {a.runs} runs gave {'identical values for every case' if all_same else 'DIFFERENT values for some cases (see the last column)'}")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
