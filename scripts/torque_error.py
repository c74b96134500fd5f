"""How far the device's torque scores are from a truth in np.longdouble, next to the float64 reference's own error:
the measurement behind the tolerance of tests/test_gpu_torque.py (tests/torque_reference.py: K, FLOOR, CAP).
For every case of the GPU test: e_gpu and e_cpu in err(x, truth) = |x - truth| / max(1, |truth|) for the three per-row
values and the torques themselves, and e_gpu / max(e_cpu, FLOOR).  K is the next power of two above the largest ratio.
usage: python scripts/torque_error.py [out]          (needs a GPU; default out: profiles/torque_error.txt)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torque_reference as tr  # noqa: E402
from gpmp2_amd import engine as E  # noqa: E402
from oracle import Oracle  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "torque_error.txt")
    eng, orc = E.Engine(), Oracle()
    lines = ["# torque scores: device vs np.longdouble truth; float64 reference (link-frame two-pass) beside it",
             "# err(x, truth) = |x - truth| / max(1, |truth|); ratio = e_gpu / max(e_cpu, 2^-52)",
             f"# {'case':18s} {'quantity':18s} {'e_gpu':>9s} {'e_cpu':>9s} {'ratio':>7s}"]
    worst, worst_gpu, worst_cpu = 0.0, 0.0, 0.0
    made = {}
    for case in tr.GPU_CASES:
        name, (N, J), B = case
        if name not in made:
            model, t = tr.models()[name](), tr.case_table(name)
            r = eng.robot(model)
            made[name] = (model, r, t, eng.dynamics(r, t["mass"], t["com"], t["inertia"], t["gravity"], t["torque"]))
        model, r, table, dyn = made[name]
        dt, traj = tr.case_dt(N), tr.case_traj(name, N, B)
        exp = tr.reference_torque_score(orc, model, table, dt, J, traj)
        truth = tr.truth_torque_score(orc, model, table, dt, J, traj)
        dev = eng.torque_score_traj(r, dyn, dt, J, traj)
        for k in tr.VALUES + ("tau",):
            e_gpu, e_cpu = tr.err(dev[k], truth[k]), tr.err(exp[k], truth[k])
            ratio = float((e_gpu / np.maximum(e_cpu, tr.FLOOR)).max())
            worst, worst_gpu, worst_cpu = max(worst, ratio), max(worst_gpu, float(e_gpu.max())), max(worst_cpu, float(e_cpu.max()))
            lines.append(f"  {tr.case_id(case):18s} {k:18s} {e_gpu.max():9.2e} {e_cpu.max():9.2e} {ratio:7.2f}")
    K = 2.0 ** int(np.floor(np.log2(worst)) + 1) if worst > 0 else 1.0
    lines.append(f"# largest e_gpu {worst_gpu:.2e}, largest e_cpu {worst_cpu:.2e}, largest ratio {worst:.2f} -> K = {K:g}"
                 f" (CAP = {tr.CAP:g}, a condition; the test has K = {tr.K:g})")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
