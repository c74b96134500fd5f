"""The measured table behind the bounds of tests/test_gpu_retime.py: per row of its trajectory cases, the distance of the
device's sdot / stamps / duration from the numpy rule (tests/retime_reference.py, fed from the same traj, ps from the
CPU oracle), as a multiple of the first clause of the bound (1e-12 relative), beside the second clause (10 x the numpy
rule's own change under a 2-ulp perturbation of traj) in the same unit, and `achieved`.  A row needs the second clause
when its first column is above 1.  Needs the GPU.  Writes profiles/retime_error.txt.

usage: python scripts/retime_error.py [--out profiles/retime_error.txt]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retime_error.txt"))
    a = ap.parse_args()
    import motion_reference as mr
    import retime_reference as rr
    import test_gpu_retime as T
    from gpmp2_amd import engine as E
    from oracle import Oracle
    eng, orc = E.Engine(), Oracle()
    lines = ["device against the numpy rule, in units of the first clause (1e-12 relative); sens: 10 x the numpy rule's change "
             "under a 2-ulp perturbation of traj, same unit; max_rate 2",
             f"{'case':<16}{'row':>4}{'sdot':>10}{'stamps':>10}{'duration':>10}{'sens sdot':>11}{'sens stamps':>12}"
             f"  {'achieved vel / acc / mid / point'}"]
    rows = second = 0
    for case in T.TRAJ_CASES:
        name, (N, J), B = case
        model = mr.models()[name]()
        r, ro = eng.robot(model), orc.robot(model)
        lim, dt = mr.case_limits(name), mr.case_dt(name)
        traj = mr.case_traj(name, N, B)
        dev = eng.retime_traj(r, T._limits(model.dof(), lim), dt, J, traj, max_rate=2.0)
        ref, _ = T._reference(orc, model, ro, lim, dt, J, traj, max_rate=2.0)
        moved, _ = T._reference(orc, model, ro, lim, dt, J, rr.ulp_perturbed(traj, np.random.default_rng(3)), max_rate=2.0)
        for b in range(B):
            col = {}
            for k in ("sdot", "stamps", "duration"):
                x, y, z = np.asarray(dev[k][b]), np.asarray(ref[b][k]), np.asarray(moved[b][k])
                unit = np.maximum(1e-12 * np.abs(y), 1e-300)
                col[k] = float(np.max(np.abs(x - y) / unit))
                col["sens " + k] = float(np.max(10.0 * np.abs(z - y) / unit))
            rows += 1
            second += max(col["sdot"], col["stamps"], col["duration"]) > 1.0
            ach = " / ".join(f"{v:.6f}" for v in dev["achieved"][b])
            lines.append(f"{mr.case_id(case):<16}{b:>4}{col['sdot']:>10.2e}{col['stamps']:>10.2e}{col['duration']:>10.2e}"
                         f"{col['sens sdot']:>11.2e}{col['sens stamps']:>12.2e}  {ach}")
    lines.append(f"rows: {rows}; rows that need the second clause: {second}")
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
