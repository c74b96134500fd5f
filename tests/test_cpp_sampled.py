"""SampledClearance of the C++ host facade (include/gpmp2mi_planner.hpp): tests/cpp/sampled_smoke.cpp compiles with plain
g++ against the C ABI and links the product library.  Without a GPU it must fail loudly; with one what it prints is what
Plan.collision_probability() gives for the same problem at the same values -- the same kernels on the same input, bit
for bit."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpmp2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "sampled_smoke.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "sampled_smoke")


def _build():
    newest = max(os.path.getmtime(p) for p in (SRC, os.path.join(ROOT, "include", "gpmp2mi_planner.hpp"),
                                               os.path.join(ROOT, "include", "gpmp2mi.h")))
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < newest:
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE,
                               "-L", CSRC, "-lgpmp2mi", f"-Wl,-rpath,{CSRC}"])
    return EXE


def _run():
    return subprocess.run([_build()], capture_output=True, text=True, timeout=300)


def test_facade_builds_and_fails_loudly_without_gpu():
    from gpmp2_amd import engine
    r = _run()
    if engine.Engine().device_count() == 0:
        assert r.returncode == 3 and "EXCEPTION" in r.stdout and "no usable HIP device" in r.stdout, r.stdout + r.stderr
    else:
        assert r.returncode == 0 and r.stdout.endswith("OK\n"), r.stdout + r.stderr


def _python_side(engine, traj):
    """the problem of sampled_smoke.cpp through the Python binding: Plan.collision_probability at `traj`"""
    import gpmp2_amd as g
    arm = g.Arm(2, [1.0, 1.0], [0.0, 0.0], [0.0, 0.0])
    model = g.ArmModel(arm, [g.BodySphere(l, 0.1, (x, 0.0, 0.0)) for l in range(2) for x in (-0.75, -0.25)])
    cells = 60
    x, y = np.meshgrid(np.arange(cells), np.arange(cells))      # field[y][x]
    field = np.hypot(-3.0 + 0.1 * x - 1.2, -3.0 + 0.1 * y - 1.0) - 0.4
    st = g.TrajOptimizerSetting(2)
    st.set_total_step(10); st.set_total_time(2.0); st.set_obs_check_inter(2); st.set_cost_sigma(0.1); st.set_epsilon(0.2)
    st.setGaussNewton()
    r, s = engine.robot(model), engine.sdf([-3.0, -3.0], 0.1, field)
    pl = engine.plan(r, s, st, 1)
    try:
        start, end, zero = np.zeros((1, 2)), np.array([[1.5, 0.5]]), np.zeros((1, 2))
        pl.set_problem(start, zero, end, zero, traj[None])
        return pl.collision_probability(3, 24, 77, required_clearance=0.05, row_first=2, sample_first=5)
    finally:
        pl.close()


@pytest.mark.gpu
def test_facade_sampled_clearance_is_that_of_plan_collision_probability(engine):
    r = _run()
    assert r.returncode == 0 and r.stdout.endswith("OK\n"), r.stdout + r.stderr
    rows = {}
    for line in r.stdout.splitlines()[:-1]:
        tag, i, *vals = line.split()
        rows[tag] = np.array([float.fromhex(v) for v in vals])
    m = _python_side(engine, rows["TRAJ"].reshape(11, 4))
    assert m["ok"][0] == 1
    print(f"hits {m['hits'][0]} of 24, probability {m['probability'][0]:.4f}")
    assert list(rows["COUNTS"]) == [m["hits"][0], m["probability"][0], m["oor_samples"][0]]
    assert np.array_equal(rows["CLEARANCE"], m["clearance"][0])
    assert np.array_equal(rows["WORST"], m["worst"][0].reshape(-1)) and np.array_equal(rows["STATEHITS"], m["state_hits"][0])
