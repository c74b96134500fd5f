"""The posterior of a solved plan on the GPU: marginal covariances and samples (include/gpmp2mi.h "posterior", the kernel
k_posterior of gpmp2_amd/csrc/posterior_kernels.hip) held to the long-double recursion of tests/posterior_reference.py.

The measure is e of that module (correlation scale, worst entry of the band, worst trajectory); for samples the same on
the sigma scale.  The bound is

    e_gpu <= min(max(K * e_cpu, FLOOR), CAP)

with e_cpu the larger of the two float64 CPU values of the SAME system, computed here (block recursion, np.linalg.inv of
the dense matrix; for samples also the float64 sampling solve): the recursion alone is occasionally lucky by 100 x.
CAP = 1e-9 is a condition, not a measurement: a relative slip of 1e-6 in one entry of one G_i must not pass
(tests/test_posterior_cpu.py: it gives 5e-9 and 7e-8).  K and FLOOR come from one measured run of every case of this
file (profiles/posterior_error.txt, written by scripts/posterior_error.py, states the rule and the run): K the next power
of two above 4 x the largest e_gpu / e_cpu, FLOOR 4 x the largest e_gpu among the cases whose e_cpu < 1e-15.

Plan-level cases gate against the ORACLE's linearization at the plan's result, the independent reference; the same
against the engine's own `linearize` is printed next to it: when only the first is large the export is at fault, when
both are the sweep.
"""
from __future__ import annotations

import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import posterior_reference as ref
from gpmp2_amd import engine as E
from gpmp2_amd import problems

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CAP = 1e-9                # no case is admitted above this, whatever K * e_cpu says
K = 32.0                  # next power of two above 4 x 4.60, the largest e_gpu / e_cpu of the measured run (planar arm, D = 4)
FLOOR = 4 * 2.049e-15     # 4 x the largest e_gpu among its cases with e_cpu < 1e-15 (chain n = 15, 2 blocks, 17 samples)
CPU_EXACT = 1e-15         # cases whose e_cpu lies below this set FLOOR

NBLKS = (1, 2, 3, 5, 17)
SAMPLE_KS = (1, 16, 17)   # one column, a full tile of columns, one past it


def bound(e_cpu):
    return min(max(K * e_cpu, FLOOR), CAP)


def _args(p):
    return p.start_conf, p.start_vel, p.end_conf, p.end_vel


# ---------------------------------------------------------------------------------------------- systems
def chain(n, nblk, B, seed):
    """B random strictly diagonally dominant (hence SPD) block-tridiagonal systems"""
    rng = np.random.default_rng(seed)
    Ho = rng.normal(size=(B, nblk - 1, n, n))
    A = rng.normal(size=(B, nblk, n, n))
    Hd = 0.5 * (A + np.swapaxes(A, -1, -2))
    for b in range(B):
        for i in range(nblk):
            off = np.abs(Hd[b, i]).sum(axis=1) - np.abs(np.diag(Hd[b, i]))
            if i > 0:
                off += np.abs(Ho[b, i - 1]).sum(axis=1)       # block (i, i-1)
            if i + 1 < nblk:
                off += np.abs(Ho[b, i]).sum(axis=0)           # block (i, i+1) = Ho[i]^T
            Hd[b, i][np.diag_indices(n)] = off + 1.0
    return Hd, Ho


def _cov_row(cid, Hd, Ho, got, own=None):
    """worst trajectory of a batch -> dict(id, e_gpu, e_cpu [, e_own])"""
    B = Hd.shape[0]
    e_gpu, e_cpu, e_own = [], [], []
    for b in range(B):
        tr = ref.truth(Hd[b], Ho[b])
        e_gpu.append(ref.cov_error(got["Sdiag"][b], got["Soff"][b], *tr))
        e_cpu.append(ref.cpu_yardstick(Hd[b], Ho[b], tr))
        if own is not None:
            e_own.append(ref.cov_error(got["Sdiag"][b], got["Soff"][b], *ref.truth(own[0][b], own[1][b])))
    w = int(np.argmax(np.array(e_gpu) / np.maximum(np.array(e_cpu), 1e-300)))
    row = dict(id=cid, e_gpu=e_gpu[w], e_cpu=e_cpu[w], worst=w)
    if own is not None:
        row["e_own"] = max(e_own)
    return row


def _sample_row(cid, Hd, Ho, z, delta):
    B = Hd.shape[0]
    e_gpu, e_cpu = [], []
    for b in range(B):
        tr = ref.truth(Hd[b], Ho[b])
        d = ref.truth_sample(Hd[b], Ho[b], z[b])
        e_gpu.append(ref.sample_error(delta[b], d, tr[0]))
        e_cpu.append(max(ref.cpu_yardstick(Hd[b], Ho[b], tr), ref.sample_error(ref.sample(Hd[b], Ho[b], z[b]), d, tr[0])))
    w = int(np.argmax(np.array(e_gpu) / np.maximum(np.array(e_cpu), 1e-300)))
    return dict(id=cid, e_gpu=e_gpu[w], e_cpu=e_cpu[w], worst=w)


# ---------------------------------------------------------------------------------------------- 1. stand-alone
def measure_chain(engine, n):
    """every nblk of NBLKS at block size n, B = 3: marginals, then samples for every K of SAMPLE_KS -> rows.  Asserts
    what does not depend on the bound: ok, exact symmetry, the NULL-output combinations."""
    rows = []
    for nblk in NBLKS:
        B = 3
        Hd, Ho = chain(n, nblk, B, 1000 * n + nblk)
        got = engine.block_tridiag_marginals(Hd, Ho)
        assert list(got["ok"]) == [1] * B
        assert np.array_equal(got["Sdiag"], np.swapaxes(got["Sdiag"], -1, -2)), "Sdiag is not exactly symmetric"
        for want in (("Sdiag",), ("Soff",), ("ok",), ("Sdiag", "ok"), ()):
            part = engine.block_tridiag_marginals(Hd, Ho, want)
            for name in ("Sdiag", "Soff", "ok"):
                assert (part[name] is None) == (name not in want)
                assert part[name] is None or np.array_equal(part[name], got[name]), (want, name)
        rows.append(_cov_row(f"chain n={n} nblk={nblk} marginals", Hd, Ho, got))
        for Ks in SAMPLE_KS:
            z = np.random.default_rng(7 * n + nblk + 100 * Ks).normal(size=(B, Ks, nblk, n))
            delta, ok = engine.block_tridiag_sample(Hd, Ho, z)
            assert list(ok) == [1] * B
            rows.append(_sample_row(f"chain n={n} nblk={nblk} samples K={Ks}", Hd, Ho, z, delta))
            if Ks == 17:      # a column does not depend on its neighbours or on the tile it rides in
                one, _ = engine.block_tridiag_sample(Hd, Ho, np.ascontiguousarray(z[:, 16:17]))
                assert np.array_equal(one[:, 0], delta[:, 16])
    return rows


def _check(rows):
    for r in rows:
        lim = bound(r["e_cpu"])
        own = f", against the engine's own linearize {r['e_own']:.2e}" if "e_own" in r else ""
        print(f"{r['id']}: e_gpu {r['e_gpu']:.2e} (trajectory {r['worst']}){own}, e_cpu {r['e_cpu']:.2e}, bound {lim:.2e}")
    for r in rows:
        lim = bound(r["e_cpu"])
        assert r["e_gpu"] <= lim, (
            f"{r['id']}: e_gpu = {r['e_gpu']:.3e} (trajectory {r['worst']}), e_cpu = {r['e_cpu']:.3e}, bound {lim:.3e}"
            + (f"; against the engine's own linearize {r['e_own']:.3e}.  Both large: the sweep; only the first: the export."
               if "e_own" in r else ""))


@pytest.mark.parametrize("n", range(1, 16))
def test_chain_marginals_and_samples(engine, n):
    _check(measure_chain(engine, n))


# ---------------------------------------------------------------------------------------------- 2. non-SPD
def test_indefinite_block_is_flagged_for_its_system_only(engine):
    n, nblk, B = 4, 3, 3
    Hd, Ho = chain(n, nblk, B, 5)
    good = engine.block_tridiag_marginals(Hd, Ho)
    z = np.random.default_rng(6).normal(size=(B, 2, nblk, n))
    dgood, _ = engine.block_tridiag_sample(Hd, Ho, z)
    bad = Hd.copy()
    bad[1, 1, 2, 2] = -1.0                 # an indefinite middle block
    got = engine.block_tridiag_marginals(bad, Ho)
    assert list(got["ok"]) == [1, 0, 1]
    delta, ok = engine.block_tridiag_sample(bad, Ho, z)
    assert list(ok) == [1, 0, 1]
    for b in (0, 2):                       # the other systems of the batch are unaffected
        assert np.array_equal(got["Sdiag"][b], good["Sdiag"][b]) and np.array_equal(got["Soff"][b], good["Soff"][b])
        assert np.array_equal(delta[b], dgood[b])
    bad[1, 1, 2, 2] = np.nan
    assert list(engine.block_tridiag_marginals(bad, Ho)["ok"]) == [1, 0, 1]


# ---------------------------------------------------------------------------------------------- 3. plans
def _wam(N):
    return problems.wam_restarts(B=3, total_step=N, obs_check_inter=2, opt="GN", sdf="40")


def _planar(D):
    from test_gpu_step_backward_error import _planar as planar
    return planar(D)


PLAN_CASES = ([(f"WAM N={N}", lambda N=N: _wam(N)) for N in (1, 2, 5, 16, 33)]
              + [(f"planar D={D}", lambda D=D: _planar(D)) for D in range(1, 8)]
              + [("config5 (Pose2)", problems.mobile_arm_config5)])


def _solved_plan(engine, p):
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pl = engine.plan(r, s, p.setting, p.B)
    pl.set_problem(*_args(p), p.init)
    pl.optimize()
    return pl, r, s


def measure_plan(engine, oracle, cid, make):
    """optimize, Plan.marginals() and Plan.sample_posterior at the result -> rows (gate: the oracle's linearization
    there; e_own: the engine's own)"""
    p = make()
    pl, r, s = _solved_plan(engine, p)
    try:
        traj = pl.result()["traj"]
        got = pl.marginals()
        assert list(got["ok"]) == [1] * p.B
        assert np.array_equal(got["Sdiag"], np.swapaxes(got["Sdiag"], -1, -2))
        z = np.random.default_rng(3).normal(size=(p.B, 2, p.setting.total_step + 1, 2 * p.setting.dof))
        delta = pl.sample_posterior(z)
        own = pl.linearize(traj)
    finally:
        pl.close()
    ro, so = oracle.robot(p.model), oracle.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    Hd, Ho, _, _ = oracle.linearize(ro, so, p.setting, *_args(p), traj)
    return [_cov_row(f"plan {cid} marginals", Hd, Ho, got, own), _sample_row(f"plan {cid} samples K=2", Hd, Ho, z, delta)]


@pytest.mark.parametrize("cid,make", [pytest.param(c, m, id=c.replace(" ", "_")) for c, m in PLAN_CASES])
def test_plan_marginals_and_samples(engine, oracle, cid, make):
    _check(measure_plan(engine, oracle, cid, make))


def test_marginals_at_an_arbitrary_trajectory(engine, oracle):
    """traj= gives the marginals there (the engine's own linearize at that trajectory is the system), and does not move
    the plan's estimate: marginals() afterwards is what it was"""
    p = _wam(5)
    pl, r, s = _solved_plan(engine, p)
    try:
        at_result = pl.marginals()
        other = p.init + 0.05 * np.random.default_rng(9).normal(size=p.init.shape)
        got = pl.marginals(other)
        Hd, Ho, _, _ = pl.linearize(other)
        again = pl.marginals()
        explicit = pl.marginals(pl.result()["traj"])
    finally:
        pl.close()
    assert list(got["ok"]) == [1] * p.B
    for b in range(p.B):
        tr = ref.truth(Hd[b], Ho[b])
        e = ref.cov_error(got["Sdiag"][b], got["Soff"][b], *tr)
        assert e <= bound(ref.cpu_yardstick(Hd[b], Ho[b], tr)), (b, e)
    assert not np.array_equal(got["Sdiag"], at_result["Sdiag"])
    for name in ("Sdiag", "Soff", "ok"):
        assert np.array_equal(again[name], at_result[name]) and np.array_equal(explicit[name], at_result[name]), name


_DEV = r"""
import numpy as np
import torch                      # torch's HIP runtime first, as bench.py does
torch.cuda.init()
from gpmp2_amd import engine as E, problems
eng = E.Engine()
p = problems.wam_restarts(B=3, total_step=5, obs_check_inter=2, opt="GN", sdf="40")
r, s = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
pl = eng.plan(r, s, p.setting, p.B)
pl.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
pl.optimize()
B, nb, n, K = p.B, p.setting.total_step + 1, 2 * p.setting.dof, 17
host = pl.marginals()
z = np.random.default_rng(4).normal(size=(B, K, nb, n))
dhost = pl.sample_posterior(z)
dev = torch.device("cuda:0")
Sd = torch.full((B, nb, n, n), float("nan"), dtype=torch.float64, device=dev)
So = torch.full((B, nb - 1, n, n), float("nan"), dtype=torch.float64, device=dev)
ok = torch.full((B,), -1, dtype=torch.int32, device=dev)
zd = torch.from_numpy(z).to(dev)
dl = torch.full((B, K, nb, n), float("nan"), dtype=torch.float64, device=dev)
ok2 = torch.full((B,), -1, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
st = torch.cuda.Stream(device=dev)
pl.marginals_dev(Sd, So, ok, stream=st.cuda_stream)
pl.sample_posterior_dev(K, zd, dl, ok2, stream=st.cuda_stream)
with torch.cuda.stream(st):
    got = [t.cpu().numpy() for t in (Sd, So, ok, dl, ok2)]
assert np.array_equal(got[0], host["Sdiag"]) and np.array_equal(got[1], host["Soff"]), "marginals_dev != marginals"
assert list(got[2]) == list(host["ok"]) == [1] * B and list(got[4]) == [1] * B
assert np.array_equal(got[3], dhost), "sample_posterior_dev != sample_posterior"
pl.marginals_dev(Sdiag=Sd, stream=st.cuda_stream)          # any output may be None
st.synchronize()
for bad in (lambda: pl.marginals_dev(Sd[:1]), lambda: pl.sample_posterior_dev(K, zd, dl[:, :1])):
    try:
        bad()
        raise SystemExit("a wrong-shape tensor was accepted")
    except ValueError:
        pass
pl.close()
print("POSTERIOR DEV OK")
"""


def test_dev_forms_equal_the_host_calls_bit_for_bit():
    """marginals_dev / sample_posterior_dev into torch tensors on a torch stream; in a fresh process that starts torch's
    HIP runtime before the library, as bench.py does"""
    assert importlib.util.find_spec("torch") is not None    # not imported here: this process keeps the library's runtime
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + [x for x in [os.environ.get("PYTHONPATH")] if x]))
    r = subprocess.run([sys.executable, "-c", _DEV], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0 and "POSTERIOR DEV OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------------------------------------- 4. replanning
def test_fix_state_pins_its_block_and_leaves_the_optimizer_alone(engine):
    p = _wam(16)
    D, k, b = p.setting.dof, 8, 1
    pl, r, s = _solved_plan(engine, p)
    twin, _, _ = _solved_plan(engine, p)
    try:
        traj = pl.result()["traj"]
        before = pl.marginals()
        for q in (pl, twin):
            q.fix_state(b, k, traj[b, k, :D], traj[b, k, D:])
        got = pl.marginals()
        z = np.random.default_rng(5).normal(size=(p.B, 1, p.setting.total_step + 1, 2 * D))
        pl.sample_posterior(z)
        Hd, Ho, _, _ = pl.linearize(traj)      # the engine's own: the oracle's linearize carries no state priors
        pl.update(1)
        twin.update(1)
        a, c = pl.result(), twin.result()
    finally:
        pl.close()
        twin.close()
    assert list(got["ok"]) == [1] * p.B
    var = np.diag(got["Sdiag"][b, k])
    s2c, s2v = p.setting.conf_prior_sigma ** 2, p.setting.vel_prior_sigma ** 2
    print(f"variances of the fixed state: x {var[:D].min():.4e} .. {var[:D].max():.4e} (prior {s2c:.1e}), "
          f"before {np.diag(before['Sdiag'][b, k])[:D].max():.2e}")
    assert np.all(np.abs(var[:D] - s2c) <= 0.01 * s2c) and np.all(np.abs(var[D:] - s2v) <= 0.01 * s2v)
    assert np.diag(before["Sdiag"][b, k])[:D].min() > 100 * s2c      # it was loose before
    for o in range(p.B):
        if o != b:     # other trajectories: bit for bit
            assert np.array_equal(got["Sdiag"][o], before["Sdiag"][o]) and np.array_equal(got["Soff"][o], before["Soff"][o])
    rows = [_cov_row("WAM N=16 after fix_state", Hd, Ho, got)]
    _check(rows)
    # update(1) after marginals / sample_posterior is update(1) without them
    for name in ("traj", "final_error", "iters", "status"):
        assert np.array_equal(a[name], c[name]), name


# ---------------------------------------------------------------------------------------------- 5. limits
def test_wide_plans_are_refused_with_the_limit_named(engine):
    from test_gpu_step_backward_error import _wide
    p = _wide(8, 10)
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pl = engine.plan(r, s, p.setting, p.B)
    try:
        pl.set_problem(*_args(p), p.init)
        z = np.zeros((p.B, 1, p.setting.total_step + 1, 16))
        fake = 8        # a device address that is never used: the refusal comes first
        for call in (lambda: pl.marginals(), lambda: pl.marginals_dev(fake, fake, fake),
                     lambda: pl.sample_posterior(z), lambda: pl.sample_posterior_dev(1, fake, fake)):
            with pytest.raises(E.Gpmp2miError) as ei:
                call()
            assert ei.value.code == 4 and "2 dof <= 15" in str(ei.value) and "dof 8" in str(ei.value), str(ei.value)
        pl.optimize()                      # the plan is as usable as before
        assert pl.result()["traj"].shape == p.init.shape
    finally:
        pl.close()


def test_bad_sample_arguments_are_invalid(engine):
    p = _wam(2)
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pl = engine.plan(r, s, p.setting, p.B)
    lib = engine.lib
    z = np.zeros((p.B, 1, 3, 14))
    d = np.zeros_like(z)
    try:
        # before set_problem there is no graph to linearize
        assert lib.gpmp2mi_plan_marginals(pl.h.ptr, None, None, None, None) == 1
        assert b"set_problem" in lib.gpmp2mi_last_error()
        pl.set_problem(*_args(p), p.init)
        assert lib.gpmp2mi_plan_sample_posterior(pl.h.ptr, 0, E.dptr(z), E.dptr(d), None) == 1
        assert lib.gpmp2mi_plan_sample_posterior(pl.h.ptr, 1, None, E.dptr(d), None) == 1
        assert lib.gpmp2mi_plan_sample_posterior(pl.h.ptr, 1, E.dptr(z), None, None) == 1
        assert lib.gpmp2mi_plan_sample_posterior_dev(pl.h.ptr, 0, ctypes.c_void_p(8), ctypes.c_void_p(8), None, None) == 1
        assert lib.gpmp2mi_plan_sample_posterior_dev(pl.h.ptr, 1, None, ctypes.c_void_p(8), None, None) == 1
        # not optimized yet: the current estimate is the initial values
        at_init, explicit = pl.marginals(), pl.marginals(p.init)
        assert np.array_equal(at_init["Sdiag"], explicit["Sdiag"]) and list(at_init["ok"]) == [1] * p.B
    finally:
        pl.close()


# ---------------------------------------------------------------------------------------------- 6. façade
def test_isam2_marginal_covariance_is_the_block_of_plan_marginals(engine):
    import gpmp2_amd as g
    p = problems.wam_restarts(B=1, total_step=10, obs_check_inter=4, sdf="40")
    sdf = g.SignedDistanceField(p.sdf_origin, p.sdf_cell, p.sdf_data.shape[1], p.sdf_data.shape[2], p.sdf_data.shape[0])
    for zi in range(p.sdf_data.shape[0]):
        sdf.initFieldData(zi, p.sdf_data[zi])
    D = p.setting.dof
    isam = g.ISAM2TrajOptimizer3DArm(p.model, sdf, p.setting)
    with pytest.raises(RuntimeError):
        isam.marginalCovariance(0)
    isam.initFactorGraph(p.start_conf[0], p.start_vel[0], p.end_conf[0], p.end_vel[0])
    isam.initValues(p.init[0])
    isam.update()
    isam.update()
    est = isam.values()
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pl = engine.plan(r, s, p.setting, 1)
    try:
        pl.set_problem(*_args(p), est[None])
        m = pl.marginals(est[None])
    finally:
        pl.close()
    for i in (0, 3, 10):
        J = isam.jointMarginalCovariance(i)
        assert J.shape == (2 * D, 2 * D) and np.array_equal(J, m["Sdiag"][0, i])
        assert np.array_equal(isam.marginalCovariance(i), J[:D, :D])
        assert np.array_equal(isam.marginalCovariance(i, velocity=True), J[D:, D:])
    with pytest.raises(IndexError):
        isam.jointMarginalCovariance(11)
    # replanning: the fixed state tightens to the prior
    isam.fixConfigAndVel(5, est[5, :D], est[5, D:])
    tight = np.diag(isam.marginalCovariance(5))
    assert np.all(np.abs(tight - p.setting.conf_prior_sigma ** 2) <= 0.01 * p.setting.conf_prior_sigma ** 2)
