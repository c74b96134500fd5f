"""The measured table behind K and FLOOR of tests/test_gpu_pose2_maps.py: every case of tests/pose2_cases.py through
the factor-level entry points on the GPU and through the oracle, each against the exact maps (tests/pose2_reference.py),
as the largest e per output and heading band.

    python scripts/pose2_maps_error.py [--lib other/libgpmp2mi.so] [--oracle other/liboracle.so] [--label branch]
        > profiles/pose2_maps_error.txt

--lib / --oracle measure another build of the two libraries (the parent's, for the before / after table); the rule for
K and FLOOR is printed with the values this run gives."""
import argparse
import ctypes as C
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from gpmp2_amd import engine  # noqa: E402
import oracle as oracle_mod  # noqa: E402
import pose2_cases as pc  # noqa: E402

CLEAN = 1e-16      # below this e_oracle is rounding of the output itself: such cases set FLOOR, the others K


def oracle_at(path):
    if path is None:
        return oracle_mod.Oracle()
    o = oracle_mod.Oracle.__new__(oracle_mod.Oracle)
    o.lib = C.CDLL(path)
    o.lib.orc_robot_destroy.argtypes = [C.c_void_p]
    o.lib.orc_sdf_destroy.argtypes = [C.c_void_p]
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=engine.LIB_PATH)
    ap.add_argument("--oracle", default=None)
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--cpu-only", action="store_true", help="the oracle's columns alone (no GPU needed)")
    a = ap.parse_args()
    orc = oracle_at(a.oracle)
    e_orc = pc.measure(orc, *pc.handles(orc))
    e_gpu = None
    if not a.cpu_only:
        eng = engine.Engine(a.lib)
        e_gpu = pc.measure(eng, *pc.handles(eng))
    cs = pc.cases()
    print(f"# {a.label}: {len(cs['prior'][0])} prior cases, {len(cs['interp'][0])} interpolation cases; "
          "e = max |got - exact| / scale per case (tests/pose2_cases.py); the largest e per output and band")
    print("# band: of the exact heading difference w (prior.*, interp.vel), of the smaller of |w| and |xi[2]| (interp.conf, obs.*)")
    print(f"# {'output':12s} {'who':7s} " + " ".join(f"{b[0]:>13s}" for b in pc.BANDS) + f" {'all':>9s}")
    for g in pc.GROUPS:
        band = pc.case_bands(g)
        for who, e in (("oracle", e_orc), ("gpu", e_gpu)):
            if e is None:
                continue
            cells = [f"{e[g][band == k].max():13.2e}" if (band == k).any() else f"{'-':>13s}" for k in range(len(pc.BANDS))]
            print(f"  {g:12s} {who:7s} " + " ".join(cells) + f" {e[g].max():9.2e}")
    if e_gpu is None:
        return
    ratio, floor, where_r, where_f = 0.0, 0.0, None, None
    for g in pc.GROUPS:
        for m, (x, y) in enumerate(zip(e_gpu[g], e_orc[g])):
            if y >= CLEAN:
                if x / y > ratio:
                    ratio, where_r = x / y, (g, m)
            elif x > floor:
                floor, where_f = x, (g, m)
    K = 2.0 ** math.ceil(math.log2(4 * ratio)) if ratio > 0 else 1.0
    if K == 4 * ratio:
        K *= 2
    print("# the rule of tests/test_gpu_pose2_maps.py: e_gpu <= min(max(K * e_oracle, FLOOR), CAP), CAP = 1e-12 a condition;")
    print(f"#   K = the next power of two above 4 x the largest e_gpu / e_oracle (over cases with e_oracle >= {CLEAN:g}),")
    print(f"#   FLOOR = 4 x the largest e_gpu among cases with e_oracle < {CLEAN:g}")
    print(f"# this run: largest ratio {ratio:.3f} at {where_r} -> K = {K:g};  largest such e_gpu {floor:.3e} at {where_f} "
          f"-> FLOOR = 4 * {floor:.3e}")
    worst = max(float(e_gpu[g].max()) for g in pc.GROUPS)
    print(f"# largest e_gpu {worst:.3e}, largest e_oracle {max(float(e_orc[g].max()) for g in pc.GROUPS):.3e}, CAP {pc.CAP:g}")


if __name__ == "__main__":
    main()
