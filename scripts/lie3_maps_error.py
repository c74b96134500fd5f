"""The measured table behind K and FLOOR of tests/test_gpu_lie3_maps.py: every case of tests/lie3_cases.py through
workspace_prior_factor and path_score_traj on the GPU and through the oracle, each against the exact maps
(tests/lie3_reference.py), as the largest e per output and angle band; then the cases at exactly pi (compared on the
group) and the targets that are not quite rotations (recorded, not gated).

    python scripts/lie3_maps_error.py [--lib other/libgpmp2mi.so] [--oracle other/liboracle.so] [--label branch]
        > profiles/lie3_maps_error.txt

--lib / --oracle measure another build of the two libraries (the parent's, for the before / after table; the path
groups' oracle column is tests/path_reference.py of the tree the script runs in); the rule for K and FLOOR is printed
with the values this run gives."""
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
import lie3_cases as lc  # noqa: E402

CLEAN = 1e-16      # below this e_oracle is rounding of the output itself: such cases set FLOOR, the others K


def oracle_at(path):
    if path is None:
        return oracle_mod.Oracle()
    o = oracle_mod.Oracle.__new__(oracle_mod.Oracle)
    o.lib = C.CDLL(path)
    o.lib.orc_robot_destroy.argtypes = [C.c_void_p]
    o.lib.orc_sdf_destroy.argtypes = [C.c_void_p]
    return o


def measure_all(impl):
    h = lc.handles(impl)
    e = lc.measure(impl, h)
    with np.errstate(all="ignore"):
        e.update(lc.measure_path(impl, h))
        return e, lc.measure_pi(impl, h), lc.measure_nonortho(impl, h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=engine.LIB_PATH)
    ap.add_argument("--oracle", default=None)
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--cpu-only", action="store_true", help="the oracle's columns alone (no GPU needed)")
    a = ap.parse_args()
    whos = [("oracle", measure_all(oracle_at(a.oracle)))]
    if not a.cpu_only:
        whos.append(("gpu", measure_all(engine.Engine(a.lib))))
    n_rot = sum(1 for c in lc.cases() if c[1] == lc.ORIENTATION)
    print(f"# {a.label}: {n_rot} orientation cases, {len(lc.cases()) - n_rot} pose cases, {len(lc.PATH_CHUNKS) * len(lc.PATH_RUNS)} "
          "path calls; e = max |got - exact| / scale per case (tests/lie3_cases.py); the largest e per output and band")
    print("# band: of the angle theta of between(des, link pose); a path call counts in the band of its largest target step")
    print(f"# {'output':12s} {'who':7s} " + " ".join(f"{b:>17s}" for b in lc.BANDS) + f" {'all':>9s}")
    for g in lc.GROUPS:
        band = lc.case_bands(g)
        for who, (e, _, _) in whos:
            cells = [f"{e[g][band == k].max():17.2e}" if (band == k).any() else f"{'-':>17s}" for k in range(len(lc.BANDS))]
            print(f"  {g:12s} {who:7s} " + " ".join(cells) + f" {e[g].max():9.2e}")
    print("# exactly pi (Rd^T Rm = diag(-1,-1,1), its two permutations, 2 a a^T - I): | |omega| - pi | in ulps, max |Exp(omega) - Rrel|")
    for who, (_, pi, _) in whos:
        print(f"  {who:7s} " + "  ".join(f"{u:.0f} ulp {d:.2e}" for u, d in pi))
    print("# des with a float32-rounded rotation block at theta = pi - 1e-6, pi - 1e-9, 1e-4, 0 (orientation, pose each): finite?, "
          "e of err and of H from the exact maps on the polar factor -- recorded, not gated")
    for who, (_, _, no) in whos:
        print(f"  {who:7s} " + "  ".join(f"{'finite' if ok else 'NOT FINITE'} {x:.1e} {y:.1e}" for ok, x, y in no))
    if len(whos) < 2:
        return
    e_orc, e_gpu = whos[0][1][0], whos[1][1][0]
    ratio, floor, where_r, where_f = 0.0, 0.0, None, None
    for g in lc.GROUPS:
        for m, (x, y) in enumerate(zip(e_gpu[g], e_orc[g])):
            if y >= CLEAN:
                if x / y > ratio:
                    ratio, where_r = x / y, (g, m)
            elif x > floor:
                floor, where_f = x, (g, m)
    K = 2.0 ** math.ceil(math.log2(4 * ratio)) if ratio > 0 else 1.0
    if K == 4 * ratio:
        K *= 2
    print("# the rule of tests/test_gpu_lie3_maps.py: e_gpu <= min(max(K * e_oracle, FLOOR), CAP), CAP = 1e-12 a condition;")
    print(f"#   K = the next power of two above 4 x the largest e_gpu / e_oracle (over cases with e_oracle >= {CLEAN:g}),")
    print(f"#   FLOOR = 4 x the largest e_gpu among cases with e_oracle < {CLEAN:g}")
    print(f"# this run: largest ratio {ratio:.3f} at {where_r} -> K = {K:g};  largest such e_gpu {floor:.3e} at {where_f} "
          f"-> FLOOR = 4 * {floor:.3e}")
    worst = max(float(e_gpu[g].max()) for g in lc.GROUPS)
    print(f"# largest e_gpu {worst:.3e}, largest e_oracle {max(float(e_orc[g].max()) for g in lc.GROUPS):.3e}, CAP {lc.CAP:g}")


if __name__ == "__main__":
    main()
