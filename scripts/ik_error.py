"""The measured table behind the bound of tests/test_gpu_ik.py: every case of that file, run `--runs` times on the GPU
against tests/ik_reference.py, with the rows whose status / iters differ, e_gpu = max |conf_gpu - conf_ref| on the rows
both converged on, d_self (the reference's own move under seeds moved by +-2 ulp) and their ratio; then the K / FLOOR
the rule gives.

    python scripts/ik_error.py [--runs 2] > profiles/ik_error.txt
"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from gpmp2_amd import engine  # noqa: E402
from oracle import Oracle  # noqa: E402
import ik_reference as ik  # noqa: E402
import test_gpu_ik as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=2)
    a = ap.parse_args()
    eng, orc = engine.Engine(), Oracle()
    ref = ik.reference(orc)
    print(f"# e_gpu = max |conf_gpu - conf_ref| of a row converged on both sides; d_self = the reference's own move of that "
          f"row under seeds moved by +-2 ulp, 4 trials (tests/ik_reference.py); {a.runs} runs")
    print(f"# {'case':18s} {'rows':>5s} {'differ':>6s} {'both':>5s} {'ref flips':>9s} {'max e_gpu':>10s} {'max d_self':>10s} "
          f"{'max ratio':>10s} {'max e_gpu, d_self<1e-15':>24s}  same in every run")
    worst_ratio, floor_e, all_same = 0.0, 0.0, True
    for c, rf, d_self, flips in ref:
        runs = [T.measure_case(eng, c, rf, d_self) for _ in range(a.runs)]
        m = runs[0]
        same = all(np.array_equal(T._bits(o["dev"][k]), T._bits(m["dev"][k])) for o in runs[1:] for k in m["dev"])
        all_same &= same
        rated = m["both"] & (m["d_self"] >= T.SELF_EXACT)
        exact = m["both"] & (m["d_self"] < T.SELF_EXACT)
        ratio = float((m["e_gpu"][rated] / m["d_self"][rated]).max()) if rated.any() else 0.0
        fl = float(m["e_gpu"][exact].max()) if exact.any() else 0.0
        worst_ratio, floor_e = max(worst_ratio, ratio), max(floor_e, fl)
        print(f"  {c.name:18s} {m['differ'].size:5d} {int(m['differ'].sum()):6d} {int(m['both'].sum()):5d} {int(flips.sum()):9d} "
              f"{m['e_gpu'].max():10.3e} {m['d_self'].max():10.3e} {ratio:10.2f} {fl:24.3e}  {'yes' if same else 'NO'}")
    K = 2.0 ** math.ceil(math.log2(4.0 * worst_ratio)) if worst_ratio > 0 else float("nan")
    if K == 4.0 * worst_ratio:
        K *= 2.0
    print(f"# largest e_gpu / d_self {worst_ratio:.3f} -> K = next power of two above 4 x that = {K:g}")
    print(f"# largest e_gpu among the rows with d_self < {T.SELF_EXACT:g}: {floor_e:.3e} -> FLOOR = 4 x that = {4.0 * floor_e:.3e}")
    print(f"# hard cap {T.CAP:g} (a condition, not measured); in the test file now: K = {T.K:g}, FLOOR = {T.FLOOR:g}")
    print(f"# the {a.runs} runs gave {'identical bits for every case' if all_same else 'DIFFERENT bits for some cases (see the last column)'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
