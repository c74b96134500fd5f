"""The seeding calls of the C++ host facade (include/gpmp2mi_planner.hpp): tests/cpp/seed_smoke.cpp compiles with plain
g++ against the C ABI and links the product library.  Without a GPU it must fail loudly; with one the restarts, results
and samples it prints are those of the Python binding for the same problem and seed, bit for bit (the same kernels on the
same input)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpmp2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "seed_smoke.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "seed_smoke")


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


@pytest.mark.gpu
def test_facade_rows_are_those_of_the_python_binding(engine):
    import gpmp2_amd as g
    from gpmp2_amd import _capi
    r = _run()
    assert r.returncode == 0 and r.stdout.endswith("OK\n"), r.stdout + r.stderr
    rows = {}
    for line in r.stdout.splitlines()[:-1]:
        tag, i, *vals = line.split()
        rows[(tag, int(i))] = np.array([float.fromhex(v) for v in vals])
    arm = g.Arm(2, [1.0, 1.0], [0.0, 0.0], [0.0, 0.0])
    model = g.ArmModel(arm, [g.BodySphere(l, 0.1, (x, 0.0, 0.0)) for l in range(2) for x in (-0.75, -0.25)])
    cells = 60
    x, y = np.meshgrid(np.arange(cells), np.arange(cells))      # field[y][x]
    field = np.hypot(-3.0 + 0.1 * x - 1.2, -3.0 + 0.1 * y - 1.0) - 0.4
    st = g.TrajOptimizerSetting(2)
    st.set_total_step(10); st.set_total_time(2.0); st.set_obs_check_inter(2); st.set_cost_sigma(0.1); st.set_epsilon(0.2)
    st.setGaussNewton()
    rb, sd = engine.robot(model), engine.sdf([-3.0, -3.0], 0.1, field)
    M, seed = 5, 77
    sc, ec, zv = np.zeros((M, 2)), np.repeat([[1.5, 0.5]], M, 0), np.zeros((M, 2))
    pl = engine.plan(rb, sd, st, 2)
    try:
        res = pl.optimize_queue_seeded(seed, sc, zv, ec, zv, scale=0.5, keep_first=True, want_init=True)
    finally:
        pl.close()
    for m in range(M):
        assert np.array_equal(rows[("INIT", m)].reshape(11, 4), res["init"][m]), m
        assert np.array_equal(rows[("TRAJ", m)].reshape(11, 4), res["traj"][m]), m
    one = engine.plan(rb, sd, st, 1)
    try:
        one.set_problem(sc[:1], zv[:1], ec[:1], zv[:1], res["traj"][:1])
        delta, ok = one.sample_posterior_seeded(3, seed)
    finally:
        one.close()
    assert ok[0] == 1
    for k in range(3):
        assert np.array_equal(rows[("DELTA", k)].reshape(11, 4), delta[0, k]), k
    assert np.array_equal(rows[("Z", 0)].reshape(3, 11, 4), engine.normal_fill(seed, _capi.RNG_POSTERIOR, 0, 1, 0, 3, 11, 4)[0])
