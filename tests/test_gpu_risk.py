"""The posterior on the executed timeline on the GPU (include/gpmp2mi.h; the kernels k_gp_interp_cov, k_risk and
k_risk_finish of gpmp2_amd/csrc/risk_kernels.hip) held to the long-double definitions of tests/risk_reference.py.

Two measures of that module, worst trajectory of a case: e_cov (correlation scale, every entry of every checked state)
and e_sig (|sigma^^2 - sigma^2| / sbar^2 over the in-range pairs).  For each the bound is

    e_gpu <= min(max(K * e_cpu, FLOOR), CAP)

with e_cpu the larger float64 CPU value of the SAME case, computed here.  CAP = 1e-9 is a condition, not a measurement:
a relative slip of 1e-6 in one interpolation scalar must not pass (tests/test_risk_cpu.py: it gives e_cov >= 1.2e-7,
e_sig >= 2.6e-8).  K and FLOOR come from one measured run of every case of this file (profiles/risk_error.txt, written by
scripts/risk_error.py, states the rule and the run): K the next power of two above 4 x the largest e_gpu / e_cpu, FLOOR
4 x the largest e_gpu among the cases whose e_cpu < 1e-15.

Stand-alone cases take a float64 band (the block recursion on the oracle's linearization) and compare with the
long-double formula on that SAME band, so only the kernels' arithmetic is measured; there e_cpu is the float64 formula.
Plan-level cases gate against long double on the ORACLE's linearization at the plan's result; e_cpu is the larger of
the two float64 compositions (recursion or dense inverse, then the float64 formula), and the same against the engine's
own `linearize` is printed next to it.

e_sig takes h = grad d . d centre / d x from the oracle in float64 for the truth and for e_cpu alike, so e_cpu holds the
rounding of the covariance only, while e_gpu also holds the device's own h.  The field gradient is a difference of
neighbouring field values divided by the cell size: one ulp of a value of 0.3 m is 30 ulp of a difference of 0.01 m, and
sigma^2 is quadratic in h.  Ratios e_gpu / e_cpu of some tens on the WAM field are that, and K_SIG below is what the
rule makes of them; CAP stays five decades above.

Cases, the smallest at which each part can go wrong: the WAM at (N, J) = (1, 5) one interval, (2, 0) support states
only, (5, 5), (16, 3) with Md = 65 -- a second tile that holds one state; the planar arms D = 1..7 at J = 2, every width
of the packed triangle and every dispatch; the point robot on a planar field at J = 1.
"""
from __future__ import annotations

import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import posterior_reference as post
import risk_reference as ref
import score_reference as sref
from gpmp2_amd import engine as E
from gpmp2_amd import problems

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CAP = 1e-9                 # no case is admitted above this, whatever K * e_cpu says
CPU_EXACT = 1e-15          # cases whose e_cpu lies below this set FLOOR
# profiles/risk_error.txt: the measured run behind these four
K_COV = 32.0              # next power of two above 4 x 4.128, the largest e_cov gpu / cpu (plan planar D=1 J=2 cov)
FLOOR_COV = 4 * 7.760e-16  # 4 x the largest e_cov of the GPU among the cases with e_cpu < 1e-15
K_SIG = 1024.0              # next power of two above 4 x 158.563, the largest e_sig gpu / cpu (WAM N=2 J=0 sigma k=0)
FLOOR_SIG = 4 * 2.295e-14  # 4 x the largest e_sig of the GPU among the cases with e_cpu < 1e-15
CLEAR_TOL = 1e-9           # the project's clearance tolerance (tests/test_gpu_score.py)


def bound(kind, e_cpu):
    K, FLOOR = (K_COV, FLOOR_COV) if kind == "cov" else (K_SIG, FLOOR_SIG)
    return min(max(K * e_cpu, FLOOR), CAP)


def _args(p):
    return p.start_conf, p.start_vel, p.end_conf, p.end_vel


# ---------------------------------------------------------------------------------------------- cases
def _wam(N):
    return problems.wam_restarts(B=3, total_step=N, obs_check_inter=2, opt="GN", sdf="40")


def _planar(D):
    from test_gpu_step_backward_error import _planar as planar
    return planar(D)


def _point():
    """the point robot of problems.point_robot_2d on its planar field, three goals"""
    p = problems.point_robot_2d()
    N, B = p.setting.total_step, 3
    start = np.tile(p.start_conf, (B, 1))
    end = p.end_conf + np.array([[0.0, 0.0], [-4.0, 1.5], [1.0, -6.0]])
    init = np.zeros((B, N + 1, 4))
    for b in range(B):
        for i in range(N + 1):
            init[b, i, :2] = start[b] * (N - i) / N + end[b] * i / N
        init[b, :, 2:] = (end[b] - start[b]) / p.setting.total_time
    z = np.zeros((B, 2))
    return problems.Problem("point robot, three goals", p.model, p.sdf_origin, p.sdf_cell, p.sdf_data, p.setting, start, z,
                            end, z.copy(), init)


CASES = ([(f"WAM N={N} J={J}", lambda N=N: _wam(N), J) for N, J in ((1, 5), (2, 0), (5, 5), (16, 3))]
         + [(f"planar D={D} J=2", lambda D=D: _planar(D), 2) for D in range(1, 8)]
         + [("point robot J=1", _point, 1)])
PARAMS = [pytest.param(c, m, J, id=c.replace(" ", "_")) for c, m, J in CASES]
KAPPAS = (0.0, 3.0)


class Ctx:
    """a problem with the oracle's handles and what every comparison of a case needs"""

    def __init__(self, oracle, p, J):
        self.p, self.J, self.D, self.B, self.N = p, J, p.setting.dof, p.B, p.setting.total_step
        self.dt = sref.delta_t(p.setting)
        self.Qc = p.setting.Qc
        self.oracle = oracle
        self.ro = oracle.robot(p.model)
        self.fld = sref.oracle_sdf(oracle, p.sdf_origin, p.sdf_cell, p.sdf_data)
        self.radius = np.asarray(p.model.flat()["sphere_radius"], dtype=np.float64)

    def linearize(self, traj):
        Hd, Ho, _, _ = self.oracle.linearize(self.ro, self.fld.handle, self.p.setting, *_args(self.p), traj)
        return Hd, Ho

    def geometry(self, traj):
        return [ref.geometry(self.oracle, self.ro, self.fld.handle, False, self.D, self.dt, self.J, traj[b],
                             self.p.sdf_origin, self.p.sdf_cell) for b in range(traj.shape[0])]


def _handles(engine, p):
    return engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)


def _worst(rows_gpu, rows_cpu):
    w = int(np.argmax(np.array(rows_gpu) / np.maximum(np.array(rows_cpu), 1e-300)))
    return rows_gpu[w], rows_cpu[w], w


def _check(rows):
    for r in rows:
        own = f", against the engine's own linearize {r['e_own']:.2e}" if "e_own" in r else ""
        print(f"{r['id']}: e_{r['kind']} gpu {r['e_gpu']:.2e} (trajectory {r['worst']}){own}, cpu {r['e_cpu']:.2e}, "
              f"bound {bound(r['kind'], r['e_cpu']):.2e}")
    for r in rows:
        lim = bound(r["kind"], r["e_cpu"])
        assert r["e_gpu"] <= lim, (f"{r['id']}: e_{r['kind']} gpu = {r['e_gpu']:.3e} (trajectory {r['worst']}), "
                                   f"cpu = {r['e_cpu']:.3e}, bound {lim:.3e}")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same_bits(a, b, names, rows_a=slice(None), rows_b=slice(None), what=""):
    for k in names:
        assert np.array_equal(_bits(a[k][rows_a]), _bits(b[k][rows_b])), (what, k)


RISK_OUT = ("robust_clearance", "worst", "sigma_worst", "out_of_range", "sigma")


def _sig_rows(cid, c, geo, cov_truth, cov_cpu, got, kappa, score=None, tag=""):
    """the comparisons of one risk answer `got` (B rows): the sigma map through e_sig, robust_clearance at the
    reference's worst pair, worst where the gap decides, out_of_range -> the e_sig row.  cov_truth: long-double dense
    covariances [B]; cov_cpu: list of float64 ones per row (every CPU composition)."""
    e_gpu, e_cpu = [], []
    bsig = None
    for b in range(c.B):
        g = geo[b]
        s2, sbar = ref.sigma_parts(g, cov_truth[b], c.D)
        # in-range pairs carry a value, the others NaN
        assert np.isfinite(got["sigma"][b][g["inr"]]).all() and np.isnan(got["sigma"][b][~g["inr"]]).all(), (cid, b)
        # A pair whose oracle centre lies within 1e-9 cells of a cell face (h != 0) may sit in the neighbouring cell on
        # the device, where the trilinear gradient is another one: such a pair is excluded when it disagrees beyond CAP
        # (a jump of the gradient is an error of order one), and at most 0.5 % of a row's pairs may be.  Near-face pairs
        # that agree stay in the measure.
        excl = g["near_face"] & (ref.sig_errors(np.where(g["inr"], got["sigma"][b], 0.0), s2, sbar) > CAP)
        print(f"  {cid}{tag} row {b}: {int(g['near_face'].sum())} pairs near a cell face, {int(excl.sum())} excluded")
        assert excl.sum() <= 0.005 * g["inr"].size, (cid, b, "pairs excluded", int(excl.sum()))
        use = g["inr"] & ~excl
        e_gpu.append(ref.e_sig(got["sigma"][b], s2, sbar, use))
        ec = 0.0
        for cc in cov_cpu[b]:
            s2c, _ = ref.sigma_parts(g, np.asarray(cc, dtype=np.float64), c.D)
            ec = max(ec, ref.e_sig(np.sqrt(np.maximum(s2c.astype(np.float64), 0)), s2, sbar, use))
        e_cpu.append(ec)
    eg, ec, w = _worst(e_gpu, e_cpu)
    row = dict(id=f"{cid} sigma{tag}", kind="sig", e_gpu=eg, e_cpu=ec, worst=w)
    bsig = bound("sig", ec)
    for b in range(c.B):
        g = geo[b]
        s2, sbar = ref.sigma_parts(g, cov_truth[b], c.D)
        r = ref.robust(g, c.radius, s2, kappa)
        if r["worst"] == (-1, -1):
            assert np.isposinf(got["robust_clearance"][b]) and tuple(got["worst"][b]) == (-1, -1), (cid, b)
            continue
        m, s = r["worst"]
        sg, sb = r["sigma_worst"], float(sbar[m, s])
        tol = CLEAR_TOL + (kappa * bsig * sb * sb / (2 * sg) if sg > 0 else kappa * np.sqrt(bsig) * sb)
        d = abs(float(got["robust_clearance"][b]) - r["c"])
        print(f"  {cid}{tag} kappa={kappa:g} row {b}: robust {got['robust_clearance'][b]:+.6f} at {tuple(got['worst'][b])}, "
              f"sigma {got['sigma_worst'][b]:.3e}; |d| {d:.1e} (tol {tol:.1e}), gap {r['gap']:.1e}")
        assert d <= tol, (cid, b, kappa, d, tol)
        if r["gap"] > 1e-6:
            assert tuple(got["worst"][b]) == r["worst"], (cid, b, kappa, got["worst"][b], r["worst"], r["gap"])
            assert abs(got["sigma_worst"][b] - sg) <= 1e-9 + np.sqrt(bsig) * sb, (cid, b)
        assert got["sigma_worst"][b] == got["sigma"][b][tuple(got["worst"][b])], (cid, b)
    if score is not None:
        assert np.array_equal(got["out_of_range"], score["out_of_range"]), (cid, got["out_of_range"], score["out_of_range"])
    return row


# ---------------------------------------------------------------------------------------------- 1, 2. stand-alone
def measure_standalone(engine, oracle, cid, make, J):
    """gp_interpolate_cov and risk_traj on a float64 band of the oracle's linearization at the initial values -> rows.
    Asserts what does not depend on the bound."""
    p = make()
    c = Ctx(oracle, p, J)
    traj = p.init
    Hd, Ho = c.linearize(traj)
    band = [post.marginals(Hd[b], Ho[b], np.float64) for b in range(c.B)]
    Sd, So = np.stack([x[0] for x in band]), np.stack([x[1] for x in band])
    truth = [ref.dense_cov(Sd[b], So[b], c.Qc, c.dt, J) for b in range(c.B)]
    cpu = [ref.dense_cov(Sd[b], So[b], c.Qc, c.dt, J, np.float64) for b in range(c.B)]
    cov = engine.gp_interpolate_cov(c.D, c.Qc, c.dt, J, Sd, So)
    assert cov.shape == (c.B, c.N * (J + 1) + 1, 2 * c.D, 2 * c.D)
    assert np.array_equal(_bits(cov), _bits(np.swapaxes(cov, -1, -2))), "cov is not exactly symmetric"
    assert np.array_equal(_bits(cov[:, ::J + 1]), _bits(Sd)), "support states are not copies of Sdiag"
    one = engine.gp_interpolate_cov(c.D, c.Qc, c.dt, J, Sd[1:2], So[1:2])
    assert np.array_equal(_bits(one[0]), _bits(cov[1])), "a row alone differs from the row in the batch"
    e_gpu = [ref.e_cov(cov[b], truth[b]) for b in range(c.B)]
    e_cpu = [ref.e_cov(cpu[b], truth[b]) for b in range(c.B)]
    eg, ec, w = _worst(e_gpu, e_cpu)
    rows = [dict(id=f"{cid} cov", kind="cov", e_gpu=eg, e_cpu=ec, worst=w)]
    # risk_traj on the same band
    r, s = _handles(engine, p)
    geo = c.geometry(traj)
    score = engine.score_traj(r, s, c.dt, J, traj)
    for kappa in KAPPAS:
        got = engine.risk_traj(r, s, c.Qc, c.dt, J, traj, Sd, So, kappa)
        rows.append(_sig_rows(cid, c, geo, truth, [[x] for x in cpu], got, kappa, score, tag=f" k={kappa:g}"))
        alone = engine.risk_traj(r, s, c.Qc, c.dt, J, traj[1:2], Sd[1:2], So[1:2], kappa)
        _same_bits(alone, got, RISK_OUT, rows_a=slice(0, 1), rows_b=slice(1, 2), what=(cid, "row alone"))
        if kappa == 0.0:
            exp = sref.oracle_score(oracle, p.model, c.ro, c.fld, c.dt, J, traj)
            assert np.abs(got["robust_clearance"] - score["min_clearance"]).max() <= 1e-12, cid
            decided = ~(exp["gap"] <= 1e-6)
            assert np.array_equal(got["worst"][decided], score["worst"][decided]), cid
            print(f"  {cid} kappa=0: robust_clearance and min_clearance "
                  f"{'agree bit for bit' if np.array_equal(_bits(got['robust_clearance']), _bits(score['min_clearance'])) else 'differ in bits'}")
    return rows


@pytest.mark.parametrize("cid,make,J", PARAMS)
def test_interpolated_covariance_and_risk_of_a_given_band(engine, oracle, cid, make, J):
    _check(measure_standalone(engine, oracle, cid, make, J))


def test_inter_step_zero_returns_the_support_blocks(engine):
    rng = np.random.default_rng(2)
    A = rng.normal(size=(2, 4, 6, 6))
    Sd = A @ np.swapaxes(A, -1, -2)
    So = rng.normal(size=(2, 3, 6, 6))
    assert np.array_equal(_bits(engine.gp_interpolate_cov(3, None, 0.3, 0, Sd, So)), _bits(Sd))


def _random_band(dof, N, B, seed):
    """a random SPD block-tridiagonal precision (the chains of test_gpu_posterior) and the float64 band of its inverse"""
    from test_gpu_posterior import chain
    Hd, Ho = chain(2 * dof, N + 1, B, seed)
    band = [post.marginals(Hd[b], Ho[b], np.float64) for b in range(B)]
    return np.stack([x[0] for x in band]), np.stack([x[1] for x in band])


def measure_wide(engine, dof):
    N, B, J, dt = 2, 3, 3, 0.25
    Sd, So = _random_band(dof, N, B, 300 + dof)
    A = np.random.default_rng(dof).normal(size=(dof, dof))
    Qc = A @ A.T + np.eye(dof)
    cov = engine.gp_interpolate_cov(dof, Qc, dt, J, Sd, So)
    assert np.array_equal(_bits(cov), _bits(np.swapaxes(cov, -1, -2))) and np.array_equal(_bits(cov[:, ::J + 1]), _bits(Sd))
    e_gpu, e_cpu = [], []
    for b in range(B):
        tr = ref.dense_cov(Sd[b], So[b], Qc, dt, J)
        e_gpu.append(ref.e_cov(cov[b], tr))
        e_cpu.append(ref.e_cov(ref.dense_cov(Sd[b], So[b], Qc, dt, J, np.float64), tr))
    eg, ec, w = _worst(e_gpu, e_cpu)
    return [dict(id=f"random band dof={dof} cov", kind="cov", e_gpu=eg, e_cpu=ec, worst=w)]


@pytest.mark.parametrize("dof", [8, 18])
def test_interpolated_covariance_needs_no_tile_layout(engine, dof):
    _check(measure_wide(engine, dof))


def test_a_row_that_is_not_spd_or_not_finite_stays_alone(engine, oracle):
    p = _wam(5)
    J, kappa = 5, 3.0
    c = Ctx(oracle, p, J)
    Hd, Ho = c.linearize(p.init)
    band = [post.marginals(Hd[b], Ho[b], np.float64) for b in range(c.B)]
    Sd, So = np.stack([x[0] for x in band]), np.stack([x[1] for x in band])
    r, s = _handles(engine, p)
    good = engine.risk_traj(r, s, c.Qc, c.dt, J, p.init, Sd, So, kappa)
    got = engine.risk_traj(r, s, c.Qc, c.dt, J, p.init, Sd, So, kappa, ok=np.array([1, 0, 1], dtype=np.int32))
    assert np.isnan(got["robust_clearance"][1]) and np.isnan(got["sigma_worst"][1]) and tuple(got["worst"][1]) == (-1, -1)
    assert got["out_of_range"][1] == good["out_of_range"][1]
    assert np.isnan(got["sigma"][1]).all()
    _same_bits(got, good, RISK_OUT, rows_a=[0, 2], rows_b=[0, 2], what="ok = 0")
    # gpmp2mi_select_best never picks the NaN row, whatever its final_error
    best, n = engine.select_best(np.array([3.0, 1.0, 2.0]), None, got["robust_clearance"], required_clearance=-1e9)
    assert (best, n) == (2, 2)
    # a NaN support state: its checked states are out of range, as gpmp2mi_score_traj counts them
    bad = p.init.copy()
    bad[1, 2, :] = np.nan
    got = engine.risk_traj(r, s, c.Qc, c.dt, J, bad, Sd, So, kappa)
    score = engine.score_traj(r, s, c.dt, J, bad)
    S = c.radius.size
    assert np.array_equal(got["out_of_range"], score["out_of_range"])
    assert got["out_of_range"][1] - good["out_of_range"][1] >= 0 and got["out_of_range"][1] >= (2 * (J + 1) - 1) * S
    assert np.isnan(got["sigma"][1, J + 2:3 * (J + 1) - 1]).all() and np.isfinite(got["robust_clearance"][1])
    _same_bits(got, good, RISK_OUT, rows_a=[0, 2], rows_b=[0, 2], what="NaN state")


# ---------------------------------------------------------------------------------------------- 3. plans
def _solved_plan(engine, p):
    r, s = _handles(engine, p)
    pl = engine.plan(r, s, p.setting, p.B)
    pl.set_problem(*_args(p), p.init)
    pl.optimize()
    return pl, r, s


def measure_plan(engine, oracle, cid, make, J, kappa=3.0):
    """optimize, Plan.marginals_dense and Plan.risk at the result -> rows (gate: long double on the oracle's
    linearization there; e_own: on the engine's own)"""
    p = make()
    c = Ctx(oracle, p, J)
    pl, r, s = _solved_plan(engine, p)
    try:
        traj = pl.result()["traj"]
        dense = pl.marginals_dense(J)
        risk = pl.risk(J, kappa)
        sup = pl.marginals()
        own = pl.linearize(traj)
        score = pl.score(J)
    finally:
        pl.close()
    assert list(dense["ok"]) == [1] * c.B and list(risk["ok"]) == [1] * c.B
    assert np.array_equal(_bits(dense["cov"][:, ::J + 1]), _bits(sup["Sdiag"])), "support blocks differ from Plan.marginals"
    assert np.array_equal(_bits(dense["cov"]), _bits(np.swapaxes(dense["cov"], -1, -2)))
    Hd, Ho = c.linearize(traj)
    truth, cpu, e_gpu, e_cpu, e_own = [], [], [], [], []
    for b in range(c.B):
        tr = ref.dense_cov(*post.truth(Hd[b], Ho[b]), c.Qc, c.dt, J)
        both = [ref.dense_cov(*x, c.Qc, c.dt, J, np.float64) for x in ref.band_float64(Hd[b], Ho[b])]
        truth.append(tr)
        cpu.append(both)
        e_gpu.append(ref.e_cov(dense["cov"][b], tr))
        e_cpu.append(max(ref.e_cov(x, tr) for x in both))
        e_own.append(ref.e_cov(dense["cov"][b], ref.dense_cov(*post.truth(own[0][b], own[1][b]), c.Qc, c.dt, J)))
    eg, ec, w = _worst(e_gpu, e_cpu)
    rows = [dict(id=f"plan {cid} cov", kind="cov", e_gpu=eg, e_cpu=ec, worst=w, e_own=max(e_own))]
    rows.append(_sig_rows(f"plan {cid}", c, c.geometry(traj), truth, cpu, risk, kappa, score))
    return rows


@pytest.mark.parametrize("cid,make,J", PARAMS)
def test_plan_dense_marginals_and_risk(engine, oracle, cid, make, J):
    _check(measure_plan(engine, oracle, cid, make, J))


def test_fix_state_tightens_sigma_and_the_optimizer_is_left_alone(engine, oracle):
    p = _wam(16)
    J, kappa, k, b = 3, 3.0, 8, 1
    c = Ctx(oracle, p, J)
    pl, r, s = _solved_plan(engine, p)
    twin, _, _ = _solved_plan(engine, p)
    try:
        traj = pl.result()["traj"]
        before = pl.risk(J, kappa)
        for q in (pl, twin):
            q.fix_state(b, k, traj[b, k, :c.D], traj[b, k, c.D:])
        after = pl.risk(J, kappa)
        pl.marginals_dense(J)
        pl.update(1)
        twin.update(1)
        x, y = pl.result(), twin.result()
    finally:
        pl.close()
        twin.close()
    m = k * (J + 1)
    h = np.asarray(c.geometry(traj[b:b + 1])[0]["h"][m], dtype=np.float64)          # [S][D]
    prior = p.setting.conf_prior_sigma * np.linalg.norm(h, axis=1)
    print(f"sigma at checked state {m} of row {b}: before {before['sigma'][b, m].max():.3e}, after "
          f"{after['sigma'][b, m].max():.3e}, prior scale {prior.max():.3e}")
    assert np.all(after["sigma"][b, m] <= 1.01 * prior + 1e-15)
    assert before["sigma"][b, m].max() > 100 * prior.max()          # it was loose before
    _same_bits(after, before, RISK_OUT, rows_a=[0, 2], rows_b=[0, 2], what="other rows after fix_state")
    for name in ("traj", "final_error", "iters", "status"):            # update(1) after the new calls = without them
        assert np.array_equal(x[name], y[name]), name


# ---------------------------------------------------------------------------------------------- 4. device forms, limits
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
B, N, n, J, kappa = p.B, p.setting.total_step, 2 * p.setting.dof, 5, 3.0
Md = N * (J + 1) + 1
dense, risk = pl.marginals_dense(J), pl.risk(J, kappa)
dev = torch.device("cuda:0")
nan = float("nan")
cov = torch.full((B, Md, n, n), nan, dtype=torch.float64, device=dev)
ok = torch.full((B,), -1, dtype=torch.int32, device=dev)
rc = torch.full((B,), nan, dtype=torch.float64, device=dev)
sw = torch.full((B,), nan, dtype=torch.float64, device=dev)
wo = torch.full((B, 2), -7, dtype=torch.int32, device=dev)
oo = torch.full((B,), -7, dtype=torch.int32, device=dev)
sg = torch.full((B, Md, r.S), 7.0, dtype=torch.float64, device=dev)
ok2 = torch.full((B,), -1, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
st = torch.cuda.Stream(device=dev)
pl.marginals_dense_dev(J, cov, ok, stream=st.cuda_stream)
pl.risk_dev(J, kappa, rc, wo, sw, oo, sg, ok2, stream=st.cuda_stream)
with torch.cuda.stream(st):
    got = [t.cpu().numpy() for t in (cov, ok, rc, wo, sw, oo, sg, ok2)]
bits = lambda a: np.ascontiguousarray(a).view(np.int64) if a.dtype == np.float64 else a
assert np.array_equal(bits(got[0]), bits(dense["cov"])), "marginals_dense_dev != marginals_dense"
assert list(got[1]) == list(dense["ok"]) == [1] * B and list(got[7]) == [1] * B
for a, name in zip(got[2:7], ("robust_clearance", "worst", "sigma_worst", "out_of_range", "sigma")):
    assert np.array_equal(bits(a), bits(risk[name])), "risk_dev != risk: " + name
pl.risk_dev(J, kappa, robust_clearance=rc, stream=st.cuda_stream)          # any output may be None
pl.marginals_dense_dev(J, ok=ok, stream=st.cuda_stream)
st.synchronize()
# the stand-alone device forms on the plan's band
m = pl.marginals()
Sd, So = torch.from_numpy(m["Sdiag"]).to(dev), torch.from_numpy(m["Soff"]).to(dev)
cov2 = torch.full((B, Md, n, n), nan, dtype=torch.float64, device=dev)
vp = lambda t: None if t is None else t.data_ptr()
rcx = eng.lib.gpmp2mi_gp_interpolate_cov_dev(n // 2, None, p.setting.total_time / N, J, B, N, vp(Sd), vp(So), vp(cov2),
                                             st.cuda_stream)
assert rcx == 0
st.synchronize()
assert np.array_equal(bits(cov2.cpu().numpy()), bits(dense["cov"])), "gp_interpolate_cov_dev != the plan's dense marginals"
pl.close()
print("RISK DEV OK")
"""


def test_dev_forms_equal_the_host_calls_bit_for_bit():
    """marginals_dense_dev / risk_dev into torch tensors on a torch stream; in a fresh process that starts torch's HIP
    runtime before the library, as bench.py does"""
    assert importlib.util.find_spec("torch") is not None    # not imported here: this process keeps the library's runtime
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + [x for x in [os.environ.get("PYTHONPATH")] if x]))
    r = subprocess.run([sys.executable, "-c", _DEV], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0 and "RISK DEV OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def _refused(engine, p, needle):
    r, s = _handles(engine, p)
    pl = engine.plan(r, s, p.setting, p.B)
    try:
        pl.set_problem(*_args(p), p.init)
        fake = 8        # a device address that is never used: the refusal comes first
        for call in (lambda: pl.marginals_dense(2), lambda: pl.marginals_dense_dev(2, fake, fake),
                     lambda: pl.risk(2, 3.0), lambda: pl.risk_dev(2, 3.0, fake, fake, fake, fake, fake, fake)):
            with pytest.raises(E.Gpmp2miError) as ei:
                call()
            assert ei.value.code == 4 and needle in str(ei.value), str(ei.value)
        pl.optimize()                      # the plan is as usable as before
        assert pl.result()["traj"].shape == p.init.shape
    finally:
        pl.close()


def test_wide_plans_are_refused_with_the_limit_named(engine):
    from test_gpu_step_backward_error import _wide
    _refused(engine, _wide(8, 10), "2 dof <= 15")


def test_pose2_plans_are_refused_with_the_missing_piece_named(engine):
    _refused(engine, problems.mobile_arm_config5(), "tangent-space interpolation")
