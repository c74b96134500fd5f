"""How far the device's coefficients of the torque rows (coef = p, m_left, m_right, tau_g of include/gpmp2mi.h "re-timing
under torque limits") are from a truth in np.longdouble, next to the float64 link-frame reference's own error: the
measurement behind K of tests/test_gpu_retime_dynamic.py.  For every case of the GPU test: e_gpu and e_cpu in
err(x, truth) = |x - truth| / max(1, |truth|) and e_gpu / max(e_cpu, FLOOR).  K is the next power of two above the largest
ratio.  Behind it, the profile: sdot, stamps and duration of the device against the numpy rule of
tests/retime_dynamic_reference.py fed the reference's coefficients and fed the device's own, in units of 1e-12 relative,
and the rows that need the sensitivity clause of the test.
usage: python scripts/retime_dynamic_error.py [out]          (needs a GPU; default out: profiles/retime_dynamic_error.txt)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import retime_dynamic_reference as dr  # noqa: E402
import torque_reference as tq  # noqa: E402
from gpmp2_amd import engine as E  # noqa: E402
from oracle import Oracle  # noqa: E402

VEL, MAX_RATE = 3.0, 4.0          # the settings of the test


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "retime_dynamic_error.txt")
    eng, orc = E.Engine(), Oracle()
    lines = ["# coefficients of the torque rows: device vs np.longdouble truth; float64 reference (link-frame two-pass) beside it",
             "# err(x, truth) = |x - truth| / max(1, |truth|); ratio = e_gpu / max(e_cpu, 2^-52)",
             f"# {'case':18s} {'quantity':10s} {'e_gpu':>9s} {'e_cpu':>9s} {'ratio':>7s}"]
    prof = ["# the profile: largest |device - numpy rule| / (1e-12 |numpy rule|) over sdot, stamps and duration of every row, with",
            "# the numpy rule fed the float64 reference's coefficients (ref) and the device's own (own); `second`: rows of the",
            "# case whose error against ref is above 1e-12 relative (they need the sensitivity clause of the test)",
            f"# {'case':18s} {'ref':>10s} {'own':>10s} {'second':>7s} {'status':>10s}"]
    worst, worst_gpu, worst_cpu, rows, second_all = 0.0, 0.0, 0.0, 0, 0
    made = {}
    for case in tq.GPU_CASES:
        name, (N, J), B = case
        if name not in made:
            model, t = tq.models()[name](), tq.case_table(name)
            r = eng.robot(model)
            made[name] = (model, r, t, eng.dynamics(r, t["mass"], t["com"], t["inertia"], t["gravity"], t["torque"]))
        model, r, table, dyn = made[name]
        D, dt, traj = model.dof(), tq.case_dt(N), tq.case_traj(name, N, B)
        exp = dr.coefficients(orc, model, table, dt, J, traj)
        truth = dr.coefficients(orc, model, table, dt, J, traj, np.longdouble)
        dev = eng.retime_dynamic_traj(r, dyn, E.MotionLimits(D, vel=VEL), dt, J, traj, max_rate=MAX_RATE)
        for i, k in enumerate(dr.COEF):
            e_gpu, e_cpu = tq.err(dev["coef"][:, :, i], truth[:, :, i]), tq.err(exp[:, :, i], truth[:, :, i])
            ratio = float((e_gpu / np.maximum(e_cpu, tq.FLOOR)).max())
            worst, worst_gpu, worst_cpu = max(worst, ratio), max(worst_gpu, float(e_gpu.max())), max(worst_cpu, float(e_cpu.max()))
            lines.append(f"  {tq.case_id(case):18s} {k:10s} {e_gpu.max():9.2e} {e_cpu.max():9.2e} {ratio:7.2f}")
        far = {"ref": 0.0, "own": 0.0}
        second = 0
        for b in range(B):
            for which, coef in (("ref", exp[b]), ("own", dev["coef"][b])):
                want = dr.retime_dynamic_traj(traj[b], coef, dr.torque_limits(table, D), dt, J, vel=np.full(D, VEL),
                                              max_rate=MAX_RATE)
                e = max(float(np.max(np.abs(np.asarray(dev[k][b]) - np.asarray(want[k])) / (1e-12 * np.abs(np.asarray(want[k])) + 1e-300)))
                        for k in ("sdot", "stamps", "duration")) if want["status"] == dr.OK else np.inf
                far[which] = max(far[which], e)
                if which == "ref":
                    second += e > 1.0
        rows += B
        second_all += second
        prof.append(f"  {tq.case_id(case):18s} {far['ref']:10.3g} {far['own']:10.3g} {second:7d} {str([int(x) for x in dev['status']]):>10s}")
    K = 2.0 ** int(np.floor(np.log2(worst)) + 1) if worst > 0 else 1.0
    lines.append(f"# largest e_gpu {worst_gpu:.2e}, largest e_cpu {worst_cpu:.2e}, largest ratio {worst:.2f} -> K = {K:g}"
                 f" (CAP = {tq.CAP:g}, a condition)")
    prof.append(f"# rows: {rows}, of which above 1e-12 relative against the reference's coefficients: {second_all}"
                f" (the test allows one in twenty)")
    text = "\n".join(lines + ["#"] + prof) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
