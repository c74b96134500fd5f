"""The measured table behind the value tolerance of tests/test_gpu_motion.py: every case of tests/motion_reference.py
(GPU_CASES, the constructed rows, the two motivation inputs solved on the device), per output
  e_gpu: the device's error against a truth evaluated in np.longdouble from the Hermite closed form (the Pose2
         interpolator with its scalars for the mobile kinds) and the oracle's Jacobians,
  e_cpu: the float64 reference's own error against that truth,
both as err(x, truth) = |x - truth| / max(1, |truth|), the worst row; then the K the rule gives.

    python scripts/motion_error.py > profiles/motion_error.txt
"""
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

from gpmp2_amd import engine as E  # noqa: E402
from oracle import Oracle  # noqa: E402
import motion_reference as mr  # noqa: E402
import score_reference as ref  # noqa: E402
import self_reference as sr  # noqa: E402


def limits(D, lim):
    return E.MotionLimits(D, **{k: v for k, v in lim.items() if v is not None})


def cases(eng, orc):
    """(id, model, robot handle, oracle handle, limits dict, dt, J, traj)"""
    made = {}

    def get(name):
        if name not in made:
            model = mr.models()[name]()
            made[name] = (model, eng.robot(model), orc.robot(model))
        return made[name]
    for c in mr.GPU_CASES:
        name, (N, J), B = c
        yield (mr.case_id(c),) + get(name) + (mr.case_limits(name), mr.case_dt(name), J, mr.case_traj(name, N, B))
    for N, J in ((8, 7), (12, 4), (12, 0)):
        yield (f"constructed-N{N}J{J}",) + get("wam") + (mr.WAM_ROUND, sr.DELTA_T, J, mr.constructed_rows(N))
    for p, J in ref.motivation_inputs():
        r, s = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
        res = eng.batch_optimize(r, s, p.setting, p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
        yield (f"motivation-B{p.B}", p.model, r, orc.robot(p.model), mr.WAM_LIMITS, ref.delta_t(p.setting), J, res["traj"])


def main():
    eng, orc = E.Engine(), Oracle()
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    print(f"# err(x, truth) = |x - truth| / max(1, |truth|), worst row of the case; on top of commit {commit or 'unknown'}")
    print(f"# rule: e_gpu <= K max(e_cpu, FLOOR) and <= CAP; FLOOR = 2^-52 (one unit in the last place of 1), K = the next")
    print(f"#       power of two above the largest e_gpu / max(e_cpu, FLOOR); in tests/motion_reference.py now: K = {mr.K:g}, "
          f"FLOOR = {mr.FLOOR:.3e}, CAP = {mr.CAP:g}")
    print(f"# {'case':24s} {'output':12s} {'e_gpu':>9s} {'e_cpu':>9s} {'ratio':>8s}  e_gpu vs float64 ref   worst agrees")
    largest = 0.0
    for cid, model, r, ro, lim, dt, J, traj in cases(eng, orc):
        D = model.dof()
        dev = eng.motion_score_traj(r, limits(D, lim), dt, J, traj)
        exp = mr.oracle_motion_score(orc, model, ro, lim, dt, J, traj)
        truth = mr.truth_motion_score(orc, model, ro, lim, dt, J, traj)
        for k in mr.VALUES:
            e_gpu, e_cpu = mr.err(dev[k], truth[k]), mr.err(exp[k], truth[k])
            ratio = (e_gpu / np.maximum(e_cpu, mr.FLOOR)).max()
            largest = max(largest, ratio)
            agree = ""
            if k in mr.KINDS:
                c = mr.KINDS.index(k)
                same = (dev["worst"][:, c] == exp["worst"][:, c]).all(axis=1)
                agree = f"{int(same.sum())}/{len(same)} rows ({int((~mr.decided(exp, c)).sum())} undecided)"
            print(f"  {cid:24s} {k:12s} {e_gpu.max():9.2e} {e_cpu.max():9.2e} {ratio:8.2f}  {mr.err(dev[k], exp[k]).max():9.2e}"
                  f"             {agree}")
        print(f"  {cid:24s} {'invalid':12s} {'equal' if np.array_equal(dev['invalid'], exp['invalid']) else 'DIFFERENT'}")
    K = 2.0 ** math.ceil(math.log2(largest)) if largest > 0 else 1.0
    if K == largest:
        K *= 2.0
    print(f"# largest e_gpu / max(e_cpu, FLOOR): {largest:.3f} -> K = {max(K, 1.0):g}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
