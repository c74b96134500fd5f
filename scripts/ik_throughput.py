"""Time of the inverse-kinematics calls against the same rule over the entry points that existed before.  New paths:
Engine.ik_solve_dev (seeded) into device buffers + a wait, Engine.ik_solve (host arrays, given seeds), Engine.ik_goals
(host arrays, no field).  Baseline: tests/ik_reference.py's iteration with Engine.workspace_prior_factor (forward
kinematics + workspace prior on the device, one round trip per iteration and pose) and numpy for the 6 x 6 solves and
the rule.  WAM, POSE mode, the limits of the tests, poses = forward kinematics of random configurations inside them, at
(G, M) = (1, 64), (1, 1 024) and (64, 256).

Every size is measured in a process of its own, started here under a time limit; the first one that fails ends the run.
Per variant the median and min / max of the per-call time over --windows windows of >= --window seconds, variants
alternated in one process, every shape warmed.  A case is accepted when the new path's median is below the baseline's
minimum.  Writes profiles/ik_throughput.json (a list, one entry per size).  --kernel-only G M: a few seeded solves and
nothing else, the target of a `rocprofv3 --kernel-trace --stats` run of its own.

usage: python scripts/ik_throughput.py [--window 0.5] [--windows 5] [--limit 400] [--out profiles/ik_throughput.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
SIZES = ((1, 64), (1, 1024), (64, 256))


class DevArray:
    """a device buffer from the library's own HIP runtime (gpmp2mi_debug_device_*): no second runtime in the process"""

    def __init__(self, eng, shape, dtype, init=None):
        self.eng, self.host = eng, np.zeros(shape, dtype=dtype)
        self.p = C.c_void_p()
        eng._ck(eng.lib.gpmp2mi_debug_device_alloc(C.c_size_t(self.host.nbytes), 0, C.byref(self.p)))
        if init is not None:
            self.host[...] = init
            eng._ck(eng.lib.gpmp2mi_debug_device_write(self.p, self.host.ctypes.data_as(C.c_void_p), C.c_size_t(self.host.nbytes)))

    @property
    def ptr(self):
        return self.p.value

    def read(self):
        self.eng._ck(self.eng.lib.gpmp2mi_debug_device_read(self.host.ctypes.data_as(C.c_void_p), self.p,
                                                            C.c_size_t(self.host.nbytes)))
        return self.host.copy()


class OverTheHost:
    """what tests/ik_reference.py asks of the oracle, answered by the engine's factor-level entry point"""

    def __init__(self, eng):
        self.eng = eng

    def workspace_prior_factor(self, robot, mode, joint, des_pose, conf):
        return self.eng.workspace_prior_factor(robot, mode, joint, des_pose, conf)


def windows(variants, window, count):
    out = {name: [] for name in variants}
    for fn in variants.values():    # warm every shape
        fn()
    for _ in range(count):
        for name, fn in variants.items():
            calls, t0 = 0, time.perf_counter()
            while True:
                fn()
                calls += 1
                if time.perf_counter() - t0 >= window:
                    break
            out[name].append((time.perf_counter() - t0) / calls)
    return out


def setup(G, M):
    import gpmp2_amd as g
    import ik_reference as ik
    from gpmp2_amd import engine
    eng = engine.Engine()
    model = g.generateArm("WAMArm")
    r = eng.robot(model)
    o = eng.ik_opts(r, limits=(ik.WAM_DOWN, ik.WAM_UP))
    rng = np.random.default_rng(17)
    q = ik.WAM_DOWN + rng.random((G, 7)) * (ik.WAM_UP - ik.WAM_DOWN)
    poses = np.ascontiguousarray(eng.forward_kinematics(r, q)[0][:, 6])
    return eng, ik, r, o, poses


def measure(G, M, window, count):
    eng, ik, r, o, poses = setup(G, M)
    seed = 5
    seeds = ik.seed_rows(seed, G, M, 0, ik.WAM_DOWN, ik.WAM_UP)
    ropts = ik.Opts(link=6, down=ik.WAM_DOWN, up=ik.WAM_UP)
    dp = DevArray(eng, (G, 16), np.float64, poses.reshape(G, 16))
    conf, res = DevArray(eng, (G, M, 7), np.float64), DevArray(eng, (G, M, 2), np.float64)
    it, st = DevArray(eng, (G, M), np.int32), DevArray(eng, (G, M), np.int32)

    def solve_dev():
        eng.ik_solve_dev(r, o, G, M, dp.ptr, seed=seed, conf=conf.ptr, residual=res.ptr, iters=it.ptr, status=st.ptr)
        eng._ck(eng.lib.gpmp2mi_debug_device_read(st.host.ctypes.data_as(C.c_void_p), st.p, C.c_size_t(4)))   # the wait

    new = eng.ik_solve(r, o, poses, seeds)
    old = ik.solve_all(OverTheHost(eng), r, ropts, poses, seeds)
    solve_dev()
    same_rows = (new["status"] == old["status"]) & (new["iters"] == old["iters"])
    both = (new["status"] == 0) & (old["status"] == 0)
    agree = bool(np.array_equal(conf.read(), new["conf"]) and same_rows.mean() >= 0.98 and
                 np.abs(new["conf"] - old["conf"])[both & same_rows].max(initial=0.0) < 1e-6)
    t = windows({"ik_solve_seeded_dev_wait": solve_dev, "ik_solve": lambda: eng.ik_solve(r, o, poses, seeds),
                 "ik_goals": lambda: eng.ik_goals(r, o, poses, seeds=seeds, radius=0.5, max_goals=8),
                 "over_the_host": lambda: ik.solve_all(OverTheHost(eng), r, ropts, poses, seeds)}, window, count)
    row = dict(G=G, M=M, mode="POSE", converged=int((new["status"] == 0).sum()), rows=G * M,
               median_iterations=float(np.median(new["iters"])), rows_equal_to_baseline=float(same_rows.mean()),
               agrees_with_host=agree)
    for name, v in t.items():
        row[name + "_ms"] = dict(median=round(1e3 * statistics.median(v), 4), min=round(1e3 * min(v), 4),
                                 max=round(1e3 * max(v), 4))
    base_min = row["over_the_host_ms"]["min"]
    row["accepted"] = {k: bool(row[k + "_ms"]["median"] < base_min) for k in ("ik_solve_seeded_dev_wait", "ik_solve", "ik_goals")}
    print(json.dumps(row), flush=True)
    return 0 if agree else 1


def kernel_only(G, M):
    eng, ik, r, o, poses = setup(G, M)
    for _ in range(5):
        eng.ik_solve(r, o, poses, M=M, seed=5)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--limit", type=int, default=400, help="seconds a size may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ik_throughput.json"))
    ap.add_argument("--size", type=int, nargs=2, metavar=("G", "M"), help="measure this size in this process")
    ap.add_argument("--kernel-only", type=int, nargs=2, metavar=("G", "M"))
    a = ap.parse_args()
    if a.kernel_only:
        return kernel_only(*a.kernel_only)
    if a.size:
        return measure(a.size[0], a.size[1], a.window, a.windows)
    rows = []
    for G, M in SIZES:   # a process and a time limit per size; the first failure ends the run
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--size", str(G),
                            str(M), "--window", str(a.window), "--windows", str(a.windows)], capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        print(r.stdout, end="", flush=True)
        lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
        if lines:
            rows.append(json.loads(lines[-1]))
        if r.returncode != 0:
            print(f"# (G, M) = ({G}, {M}): exit status {r.returncode}; stopped here", flush=True)
            break
    with open(a.out, "w") as fh:
        json.dump(rows, fh, indent=1)
        fh.write("\n")
    return 0 if len(rows) == len(SIZES) else 1


if __name__ == "__main__":
    sys.exit(main())
