"""The measured table behind the bounds of tests/test_gpu_seed.py: every bounded case of that file run once on the GPU --
the normals against the numpy restatement, H_seed against the oracle, the restarts against the long-double recursion (and,
for information, the seeded posterior of solved WAM plans, which is held to the bound of tests/test_gpu_posterior.py) --
then the constants the stated rules give.

    python scripts/seed_error.py          # writes profiles/seed_error.txt
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from gpmp2_amd import engine  # noqa: E402
from oracle import Oracle  # noqa: E402
import test_gpu_seed as T  # noqa: E402


def pow2_above(x):
    """the next power of two above x"""
    p = 2.0 ** math.ceil(math.log2(x))
    return p * 2.0 if p == x else p


def main():
    eng, orc = engine.Engine(), Oracle()
    out = []
    say = out.append
    say("# scripts/seed_error.py: one run of every bounded case of tests/test_gpu_seed.py")
    say("#")
    say("# 1. normal_fill against tests/rng_reference.py (float64 numpy on the same integers): largest |difference|")
    fill = T.measure_fill(eng)
    for r in fill:
        say(f"  {r['id']:52s} {r['diff']:9.2e}")
    zmax = max(r["diff"] for r in fill)
    ztol = min(pow2_above(4 * zmax), T.Z_CAP) if zmax > 0 else 0.0
    say(f"# largest {zmax:.3e} -> Z_TOL = next power of two above 4 x that = {pow2_above(4 * zmax) if zmax > 0 else 0.0:.3e}"
        f" = 2^{math.log2(pow2_above(4 * zmax)) if zmax > 0 else float('nan'):.0f}, capped at {T.Z_CAP:g}: {ztol:.3e}")
    say("#")
    say("# 2. H_seed against the oracle's linearization over the constant-1000 field: worst |H - H_oracle| / max |block|")
    hmax = 0.0
    for cid, make in T.PRIOR_CASES:
        row, _, _ = T.measure_prior(eng, orc, cid, make)
        hmax = max(hmax, row["err"])
        say(f"  {cid:52s} {row['err']:9.2e}")
    say(f"# largest {hmax:.3e} -> H_TOL = next power of two above 4 x that = {pow2_above(4 * hmax) if hmax > 0 else 0.0:.3e}"
        f" = 2^{math.log2(pow2_above(4 * hmax)) if hmax > 0 else float('nan'):.0f}, capped at {T.H_CAP:g}")
    say("#")
    say("# 3. restarts against the long-double recursion on H_seed, sigma scale (measure of tests/posterior_reference.py)")
    say(f"# {'case':50s} {'e_gpu':>9s} {'e_cpu':>9s} {'ratio':>8s}")
    worst, floor_e = 0.0, 0.0
    for cid, make in T.PRIOR_CASES:
        for r in T.measure_restarts(eng, cid, make):
            ratio = r["e_gpu"] / r["e_cpu"] if r["e_cpu"] > 0 else float("inf")
            worst = max(worst, ratio)
            if r["e_cpu"] < T.CPU_EXACT:
                floor_e = max(floor_e, r["e_gpu"])
            say(f"  {r['id']:50s} {r['e_gpu']:9.2e} {r['e_cpu']:9.2e} {ratio:8.2f}")
    say(f"# largest e_gpu / e_cpu {worst:.3f} -> K = next power of two above 4 x that = {pow2_above(4 * worst):g}")
    say(f"# largest e_gpu among the cases with e_cpu < {T.CPU_EXACT:g}: {floor_e:.3e} -> FLOOR = 4 x that = {4 * floor_e:.3e}")
    say(f"# hard cap {T.CAP:g} (a condition, not measured)")
    say("#")
    say("# 4. seeded posterior of solved WAM plans (bound: tests/test_gpu_posterior.py, K = %g, FLOOR = %.3e)" % (T.TP.K, T.TP.FLOOR))
    say("# e_same: seeded - unseeded kernel on the same z, sigma scale (bound: that of section 3 at the case's e_cpu)")
    say(f"# {'case':50s} {'e_gpu':>9s} {'e_cpu':>9s} {'ratio':>8s} {'unseeded':>9s} {'e_same':>9s}  bit-identical")
    for N in (1, 5, 16):
        for r in T.measure_posterior(eng, N):
            ratio = r["e_gpu"] / r["e_cpu"] if r["e_cpu"] > 0 else float("inf")
            say(f"  {r['id']:50s} {r['e_gpu']:9.2e} {r['e_cpu']:9.2e} {ratio:8.2f} {r['e_plain']:9.2e} {r['e_same']:9.2e}  {'yes' if r['same'] else 'NO'}")
    text = "\n".join(out) + "\n"
    with open(os.path.join(ROOT, "profiles", "seed_error.txt"), "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
