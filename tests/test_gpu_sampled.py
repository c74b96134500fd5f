"""The sampled clearance on the GPU (include/gpmp2mi.h "sampled clearance"; the kernels k_sampled_clearance and
k_sampled_finish of gpmp2_amd/csrc/sample_clearance_kernels.hip) held to the definitions of tests/sampled_reference.py.

Accuracy is gated on the per-(sample, state) maps, never on the row's minimum alone (tests/test_sampled_cpu.py shows why):
e_conf = max |conf - ref| and e_clr = max |state_clearance - ref| over the finite entries, the +inf patterns equal.  For
each the bound is

    e_gpu <= min(max(K_f * e_cpu, FLOOR), CAP)

with e_cpu the float64 spread of the SAME case (the reference on float64 support samples against the same on long-double
ones, sampled_cases.Ctx.spread).  CAP = 1e-9 is a condition, not a measurement: a relative slip of 1e-6 in one entry of
the bridge factor or in the support samples must not pass (tests/test_sampled_cpu.py).  K_f and FLOOR come from one
measured run of every case of this file (profiles/sampled_error.txt, written by scripts/sampled_error.py, states the rule
and the run): K_f the next power of two above 4 x the largest e_gpu / e_cpu among the cases whose e_cpu is resolved
(>= 2^-52, one ulp of unity: with both states pinned the spread is one ulp of a coordinate that is nearly zero, 2.7e-20,
and a ratio to it measures nothing), FLOOR 4 x the largest e_gpu among the cases whose e_cpu < 1e-15.

Stand-alone cases hand the device float64 support samples and compare with the reference on those SAME samples, so only
the kernels' arithmetic is measured.  Plan-level cases gate against long-double samples of the ORACLE's linearization at
the plan's result.

Counts are compared through the bound: with T the threshold, #(ref < T - bound) <= hits <= #(ref < T + bound), and the same
per state; a case whose bound leaves a reference value undecided fails.  What follows from the call's own outputs is
compared exactly.
"""
from __future__ import annotations

import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import sampled_cases as cases
import sampled_reference as ref
import score_reference as sref
from gpmp2_amd import engine as E
from gpmp2_amd import problems

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CAP = ref.CAP              # no case is admitted above this, whatever K_f * e_cpu says
CPU_EXACT = 1e-15          # cases whose e_cpu lies below this set FLOOR
RESOLVED = 2.0 ** -52      # a spread below one ulp of unity is not resolved on maps of size one: it sets FLOOR, no ratio
# profiles/sampled_error.txt: the measured run behind these four
K_CONF = 1024.0            # next power of two above 4 x 150.07, the largest e_conf gpu / cpu (wam N=2 J=63 bridge=1)
FLOOR_CONF = 4 * 6.665e-14  # 4 x the largest e_conf of the GPU among the cases with e_cpu < 1e-15 (the same case)
K_CLR = 1024.0             # next power of two above 4 x 233.62, the largest e_clr gpu / cpu (wam N=2 J=63 bridge=1)
FLOOR_CLR = 4 * 1.038e-13  # 4 x the largest e_clr of the GPU among the cases with e_cpu < 1e-15 (the same case)

PARAMS = [pytest.param(r, N, J, id=f"{r}_N{N}_J{J}") for r, N, J in cases.ALL]
OUT = ("hits", "probability", "clearance", "worst", "state_clearance", "state_hits", "oor_samples")


def bound(kind, e_cpu):
    K, FLOOR = (K_CONF, FLOOR_CONF) if kind == "conf" else (K_CLR, FLOOR_CLR)
    return min(max(K * e_cpu, FLOOR), CAP)


def _args(p):
    return p.start_conf, p.start_vel, p.end_conf, p.end_vel


def _handles(engine, p):
    return engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same_bits(a, b, names, rows_a=slice(None), rows_b=slice(None), what=""):
    for k in names:
        assert np.array_equal(_bits(a[k][rows_a]), _bits(b[k][rows_b])), (what, k)


def _own_outputs_agree(o, T, K, what):
    """what follows exactly from the call's own outputs, whatever the bound"""
    clr, st = o["clearance"], o["state_clearance"]
    assert np.array_equal(o["hits"], (clr < T).sum(axis=1)), (what, "hits")
    assert np.array_equal(o["state_hits"], (st < T).sum(axis=1)), (what, "state_hits")
    assert np.array_equal(_bits(clr), _bits(st.min(axis=2))), (what, "clearance is not the row minimum of the map")
    assert np.array_equal(_bits(o["probability"]), _bits(o["hits"] / np.float64(K))), (what, "probability")
    for b in range(clr.shape[0]):
        for s in range(K):
            m, sp = o["worst"][b, s]
            if np.isposinf(clr[b, s]):
                assert (m, sp) == (-1, -1), (what, b, s)
            else:
                assert sp >= 0 and st[b, s, m] == clr[b, s] and m == int(np.argmin(st[b, s])), (what, b, s, m)


def _counts_within(o, rows, T, bnds, K, what):
    for b, r in enumerate(rows):
        state, bnd = r["state"][:K], bnds[b]
        lo, hi = ref.counts(state, T, -bnd), ref.counts(state, T, +bnd)
        assert hi["undecided"] == 0, (what, b, "the bound leaves reference values undecided", hi["undecided"], bnd)
        assert lo["hits"] <= o["hits"][b] <= hi["hits"], (what, b, o["hits"][b], lo["hits"], hi["hits"])
        assert np.all(lo["state_hits"] <= o["state_hits"][b]) and np.all(o["state_hits"][b] <= hi["state_hits"]), (what, b)
        assert o["oor_samples"][b] == int(r["oor"][:K].sum()), (what, b, "oor_samples")


# ---------------------------------------------------------------------------------------------- 1. stand-alone
def measure_standalone(engine, oracle, robot, N, J):
    """every stand-alone call of one (robot, N, J) against the reference -> rows of (id, kind, e_gpu, e_cpu, worst).
    Asserts what does not depend on the bound; `check_counts(rows)` afterwards asserts what does."""
    c = cases.ctx(oracle, robot, N, J)
    r, s = _handles(engine, c.p)
    rows, later = [], []
    for bridge in (0, 1):
        cid = f"{robot} N={N} J={J} bridge={bridge}"
        refs = [c.row(b, bridge) for b in range(cases.B)]
        call = lambda K, T: engine.sampled_clearance_traj(
            r, s, c.Qc, c.dt, J, c.est, c.delta[:, :K], c.seed, T, row_first=cases.ROW_FIRST,
            sample_first=cases.SAMPLE_FIRST, bridge=bridge, want_conf=True)
        full = call(cases.K_REF, ref.T_MAP)
        e = [ref.map_errors(full["conf"][b], full["state_clearance"][b], refs[b]) for b in range(cases.B)]
        spread = [c.spread(b, bridge) for b in range(cases.B)]
        for k, kind in enumerate(("conf", "clr")):
            eg, ec = [x[k] for x in e], [x[k] for x in spread]
            w = int(np.argmax(np.array(eg) / np.maximum(np.array(ec), 1e-300)))
            rows.append(dict(id=cid, kind=kind, e_gpu=eg[w], e_cpu=ec[w], worst=w))
        _own_outputs_agree(full, ref.T_MAP, cases.K_REF, cid)
        own = [x[1] for x in spread]                   # each row's own e_cpu of the clearance map: its count brackets
        later.append((cid, full, refs, ref.T_MAP, cases.K_REF, own))
        for b in range(cases.B):                       # each row's own median threshold
            T = ref.t_med(refs[b]["clearance"])
            o = call(cases.K_REF, T)
            _own_outputs_agree(o, T, cases.K_REF, (cid, "T_med of row", b))
            _same_bits(o, full, ("clearance", "worst", "state_clearance", "conf"), what=(cid, "the threshold moved a map"))
            later.append((f"{cid} T_med row {b}", dict(o, only=b), refs, T, cases.K_REF, own))
        for K in cases.KS[:-1]:                        # K = 1, 16: the prefixes of the 17 samples, bit for bit
            o = call(K, ref.T_MAP)
            _own_outputs_agree(o, ref.T_MAP, K, (cid, "K", K))
            for name in ("clearance", "worst", "state_clearance", "conf"):
                assert np.array_equal(_bits(o[name]), _bits(full[name][:, :K])), (cid, "K", K, name)
            later.append((f"{cid} K={K}", o, refs, ref.T_MAP, K, own))
    return rows, later


def check_counts(later):
    """the count brackets of every call, each row under the bound of its own e_cpu"""
    for cid, o, refs, T, K, e_cpu in later:
        bnds = [bound("clr", e) for e in e_cpu]
        if "only" in o:
            b = o["only"]
            sub = {k: o[k][b:b + 1] for k in ("hits", "state_hits", "oor_samples")}
            _counts_within(sub, refs[b:b + 1], T, bnds[b:b + 1], K, cid)
        else:
            _counts_within(o, refs, T, bnds, K, cid)


def _check(rows):
    for r in rows:
        print(f"{r['id']}: e_{r['kind']} gpu {r['e_gpu']:.2e} (row {r['worst']}), cpu {r['e_cpu']:.2e}, "
              f"bound {bound(r['kind'], r['e_cpu']):.2e}")
    for r in rows:
        lim = bound(r["kind"], r["e_cpu"])
        assert r["e_gpu"] <= lim, (f"{r['id']}: e_{r['kind']} gpu = {r['e_gpu']:.3e} (row {r['worst']}), "
                                   f"cpu = {r['e_cpu']:.3e}, bound {lim:.3e}")


@pytest.mark.parametrize("robot,N,J", PARAMS)
def test_standalone_call_against_the_reference(engine, oracle, robot, N, J):
    rows, later = measure_standalone(engine, oracle, robot, N, J)
    _check(rows)
    check_counts(later)


# ---------------------------------------------------------------------------------------------- 2. scoring identity
@pytest.mark.parametrize("robot,N,J", [("wam", 5, 0), ("wam", 5, 3), ("planar", 5, 0), ("planar", 5, 3), ("point", 33, 3)])
def test_without_the_bridge_a_sample_scores_as_score_traj_does(engine, oracle, robot, N, J):
    """bridge = 0 (and J = 0 with any bridge): clearance and worst are those of gpmp2mi_score_traj(traj + delta), bit for
    bit, per sample"""
    c = cases.ctx(oracle, robot, N, dict(cases.NJ)[N])           # a shared case: the samples do not depend on J
    r, s = _handles(engine, c.p)
    for bridge in ((0, 1) if J == 0 else (0,)):
        o = engine.sampled_clearance_traj(r, s, c.Qc, c.dt, J, c.est, c.delta, c.seed, 0.0, bridge=bridge,
                                          row_first=cases.ROW_FIRST, sample_first=cases.SAMPLE_FIRST)
        for b in range(cases.B):
            zeta = c.est[b][None] + c.delta[b]
            sc = engine.score_traj(r, s, c.dt, J, zeta)
            assert np.array_equal(_bits(o["clearance"][b]), _bits(sc["min_clearance"])), (robot, J, b, bridge)
            assert np.array_equal(o["worst"][b], sc["worst"]), (robot, J, b, bridge)
            assert np.array_equal(o["oor_samples"][b], (sc["out_of_range"] > 0).sum()), (robot, J, b)


# ---------------------------------------------------------------------------------------------- 3. plans
def _solved_plan(engine, p):
    r, s = _handles(engine, p)
    pl = engine.plan(r, s, p.setting, p.B)
    pl.set_problem(*_args(p), p.init)
    pl.optimize()
    return pl, r, s


def measure_plan(engine, oracle, robot, N, J, K=cases.K_REF):
    p = cases.MAKE[robot](N)
    dt, D, Qc = sref.delta_t(p.setting), p.setting.dof, p.setting.Qc
    pl, r, s = _solved_plan(engine, p)
    rf, sf = cases.ROW_FIRST, cases.SAMPLE_FIRST
    try:
        traj = pl.result()["traj"]
        got = pl.collision_probability(J, K, cases.SEED, ref.T_MAP, row_first=rf, sample_first=sf)
        delta, ok = pl.sample_posterior_seeded(K, cases.SEED, row_first=rf, sample_first=sf)
        conf, ok2 = pl.sample_dense_seeded(J, K, cases.SEED, row_first=rf, sample_first=sf)
        plain = pl.sample_dense_seeded(J, K, cases.SEED, row_first=rf, sample_first=sf, bridge=False)[0]
    finally:
        pl.close()
    assert list(got["ok"]) == [1] * p.B and list(ok) == [1] * p.B and list(ok2) == [1] * p.B
    alone = engine.sampled_clearance_traj(r, s, Qc, dt, J, traj, delta, cases.SEED, ref.T_MAP, ok=ok, row_first=rf,
                                          sample_first=sf, want_conf=True)
    _same_bits(got, alone, OUT, what=(robot, "Plan.collision_probability != the stand-alone call on its samples"))
    assert np.array_equal(_bits(conf), _bits(alone["conf"])), "Plan.sample_dense_seeded != conf of the stand-alone call"
    assert np.abs(conf - plain)[:, :, ::J + 1].max() == 0 and np.abs(conf - plain).max() > 1e-4, "the bridge is missing"
    _own_outputs_agree(got, ref.T_MAP, K, (robot, "plan"))
    # against the reference at the oracle's linearization, long-double support samples
    ro, fld = oracle.robot(p.model), sref.oracle_sdf(oracle, p.sdf_origin, p.sdf_cell, p.sdf_data)
    radius = np.asarray(p.model.flat()["sphere_radius"], dtype=np.float64)
    Hd, Ho, _, _ = oracle.linearize(ro, fld.handle, p.setting, *_args(p), traj)
    e_gpu, e_cpu, refs = [], [], []
    for b in range(p.B):
        run = lambda dtype: ref.row(oracle, ro, fld, radius, Qc, D, dt, J, traj[b],
                                    ref.support_samples(Hd[b], Ho[b], cases.SEED, rf + b, sf, K, dtype), cases.SEED, rf + b, sf)
        truth, f64 = run(ref.LD), run(np.float64)
        refs.append(truth)
        e_gpu.append(ref.map_errors(conf[b], got["state_clearance"][b], truth))
        fin = np.isfinite(truth["state"]) & np.isfinite(f64["state"])
        e_cpu.append((float(np.abs(truth["conf"].astype(np.float64) - f64["conf"].astype(np.float64)).max()),
                      float(np.abs(truth["state"][fin] - f64["state"][fin]).max())))
    rows = []
    for k, kind in enumerate(("conf", "clr")):
        eg, ec = [x[k] for x in e_gpu], [x[k] for x in e_cpu]
        w = int(np.argmax(np.array(eg) / np.maximum(np.array(ec), 1e-300)))
        rows.append(dict(id=f"plan {robot} N={N} J={J}", kind=kind, e_gpu=eg[w], e_cpu=ec[w], worst=w))
    return rows, [(f"plan {robot}", got, refs, ref.T_MAP, K, [x[1] for x in e_cpu])]


@pytest.mark.parametrize("robot,N,J", [("wam", 5, 5), ("planar", 5, 5)])
def test_plan_form_is_the_standalone_call_on_the_plans_samples(engine, oracle, robot, N, J):
    rows, later = measure_plan(engine, oracle, robot, N, J)
    _check(rows)
    check_counts(later)


# ---------------------------------------------------------------------------------------------- 4. determinism
def test_outputs_do_not_depend_on_the_split_the_batch_or_the_chunk(engine, oracle):
    p = cases.wam(5)
    J, T, seed = 5, ref.T_MAP, cases.SEED
    pl, r, s = _solved_plan(engine, p)
    maps = ("clearance", "worst", "state_clearance")
    try:
        whole = pl.collision_probability(J, 40, seed, T, sample_first=2)
        a = pl.collision_probability(J, 17, seed, T, sample_first=2)
        b = pl.collision_probability(J, 23, seed, T, sample_first=19)
        for k in maps:
            assert np.array_equal(_bits(whole[k]), _bits(np.concatenate([a[k], b[k]], axis=1))), ("17 + 23", k)
        for k in ("hits", "state_hits", "oor_samples"):
            assert np.array_equal(whole[k], a[k] + b[k]), ("17 + 23", k)
        engine.sampled_chunk_bytes(1)                       # one 16-sample chunk: 16 + 16 + 8
        try:
            small = pl.collision_probability(J, 40, seed, T, sample_first=2)
            conf_small = pl.sample_dense_seeded(J, 40, seed, sample_first=2)[0]
        finally:
            engine.sampled_chunk_bytes(0)
        _same_bits(small, whole, OUT + ("ok",), what="one 16-sample chunk")
        assert np.array_equal(_bits(conf_small), _bits(pl.sample_dense_seeded(J, 40, seed, sample_first=2)[0]))
        traj = pl.result()["traj"]
        delta, ok = pl.sample_posterior_seeded(40, seed, sample_first=2)
    finally:
        pl.close()
    Qc, dt = p.setting.Qc, sref.delta_t(p.setting)
    batch = engine.sampled_clearance_traj(r, s, Qc, dt, J, traj, delta, seed, T, sample_first=2, want_conf=True)
    _same_bits(batch, whole, OUT, what="stand-alone on the plan's samples")
    one = engine.sampled_clearance_traj(r, s, Qc, dt, J, traj[1:2], delta[1:2], seed, T, row_first=1, sample_first=2,
                                        want_conf=True)
    _same_bits(one, batch, OUT + ("conf",), rows_a=slice(0, 1), rows_b=slice(1, 2), what="row 1 alone")


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
B, N, D, J, K, T, seed = p.B, p.setting.total_step, p.setting.dof, 5, 24, 0.08, 99
Md = N * (J + 1) + 1
host = pl.collision_probability(J, K, seed, T, row_first=1, sample_first=4)
hconf, _ = pl.sample_dense_seeded(J, K, seed, row_first=1, sample_first=4)
dev = torch.device("cuda:0")
f = lambda shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
i = lambda shape: torch.full(shape, -7, dtype=torch.int32, device=dev)
o = dict(hits=i((B,)), probability=f((B,)), clearance=f((B, K)), worst=i((B, K, 2)), state_clearance=f((B, K, Md)),
         state_hits=i((B, Md)), oor_samples=i((B,)), ok=i((B,)))
conf, ok2 = f((B, K, Md, D)), i((B,))
torch.cuda.synchronize()
st = torch.cuda.Stream(device=dev)
pl.collision_probability_dev(J, K, seed, T, row_first=1, sample_first=4, stream=st.cuda_stream, **o)
pl.sample_dense_seeded_dev(J, K, seed, conf, ok2, row_first=1, sample_first=4, stream=st.cuda_stream)
with torch.cuda.stream(st):
    got = {k: v.cpu().numpy() for k, v in o.items()}
    gconf = conf.cpu().numpy()
bits = lambda a: np.ascontiguousarray(a).view(np.int64) if a.dtype == np.float64 else a
for k in got:
    assert np.array_equal(bits(got[k]), bits(host[k])), "collision_probability_dev != collision_probability: " + k
assert np.array_equal(bits(gconf), bits(hconf)), "sample_dense_seeded_dev != sample_dense_seeded"
pl.collision_probability_dev(J, K, seed, T, hits=o["hits"], stream=st.cuda_stream)       # any output may be None
st.synchronize()
# the stand-alone device form on the plan's samples
traj = torch.from_numpy(pl.result()["traj"]).to(dev)
delta, ok = pl.sample_posterior_seeded(K, seed, row_first=1, sample_first=4)
delta = torch.from_numpy(delta).to(dev)
clr, hits = f((B, K)), i((B,))
Qc = np.ascontiguousarray(p.setting.Qc, dtype=np.float64)
rc = eng.lib.gpmp2mi_sampled_clearance_traj_dev(r.ptr, s.ptr, E.dptr(Qc), p.setting.total_time / N, J, B, N, K,
        traj.data_ptr(), delta.data_ptr(), None, seed, 1, 4, 1, T, hits.data_ptr(), None, clr.data_ptr(), None, None, None,
        None, None, st.cuda_stream)
assert rc == 0, eng.lib.gpmp2mi_last_error()
st.synchronize()
assert np.array_equal(bits(clr.cpu().numpy()), bits(host["clearance"])) and np.array_equal(hits.cpu().numpy(), host["hits"])
pl.close()
print("SAMPLED DEV OK")
"""


def test_dev_forms_equal_the_host_calls_bit_for_bit():
    """the `_dev` forms into torch tensors on a torch stream; in a fresh process that starts torch's HIP runtime before
    the library, as bench.py does"""
    assert importlib.util.find_spec("torch") is not None    # not imported here: this process keeps the library's runtime
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + [x for x in [os.environ.get("PYTHONPATH")] if x]))
    r = subprocess.run([sys.executable, "-c", _DEV], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0 and "SAMPLED DEV OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------------------------------------- 5. statistics
def statistics_bounds(conf, mean, var, K):
    """per checked state and coordinate: |sample mean - mean| / (sigma / sqrt K) and |sample variance / var - 1| /
    sqrt(2 / K); both must stay below 5"""
    m, v = conf.mean(axis=0), conf.var(axis=0, ddof=1)
    return np.abs(m - mean) / np.sqrt(var / K), np.abs(v / var - 1.0) / np.sqrt(2.0 / K)


def test_sample_moments_are_those_of_the_dense_marginals(engine):
    """WAM (5, 5), row 0, K = 4 096: the mean of conf is the interpolated estimate and its variances are the diagonal of
    Sigma_xx(m) of Plan.marginals_dense, the sub-steps where the bridge term dominates included; without the bridge the
    variance is too small in the middle of an interval"""
    p = cases.wam(5)
    J, K, D = 5, 4096, 7
    pl, r, s = _solved_plan(engine, p)
    try:
        conf = pl.sample_dense_seeded(J, K, 4242)[0][0]
        plain = pl.sample_dense_seeded(J, K, 4242, bridge=False)[0][0]
        cov = pl.marginals_dense(J)["cov"][0]
        traj = pl.result()["traj"]
    finally:
        pl.close()
    mean = engine.interpolate_traj(D, False, p.setting.Qc, sref.delta_t(p.setting), J, traj[0:1])[0][:, :D]
    var = np.diagonal(cov[:, :D, :D], axis1=1, axis2=2)
    zm, zv = statistics_bounds(conf, mean, var, K)
    print(f"with the bridge: mean {zm.max():.2f} sigma / sqrt K, variance {zv.max():.2f} sqrt(2 / K)")
    assert zm.max() < 5 and zv.max() < 5
    _, zv0 = statistics_bounds(plain, mean, var, K)
    sub = np.arange(conf.shape[1]) % (J + 1)
    print(f"without: variance {zv0[sub == (J + 1) // 2].max():.2f} sqrt(2 / K) at the mid-interval sub-steps")
    assert zv0[sub == (J + 1) // 2].max() > 5 and zv0[sub == 0].max() < 5


# ---------------------------------------------------------------------------------------------- 6. state rules
def test_a_row_that_is_not_spd_stays_alone(engine, oracle):
    c = cases.ctx(oracle, "wam", 5, 5)
    r, s = _handles(engine, c.p)
    K, T = cases.K_REF, ref.T_MAP
    call = lambda delta, ok: engine.sampled_clearance_traj(r, s, c.Qc, c.dt, c.J, c.est, delta, cases.SEED, T, ok=ok,
                                                           row_first=cases.ROW_FIRST, sample_first=cases.SAMPLE_FIRST,
                                                           want_conf=True)
    good = call(c.delta, None)
    bad = c.delta.copy()
    bad[1] = np.nan
    got = call(bad, np.array([1, 0, 1], dtype=np.int32))
    assert got["hits"][1] == -1 and got["oor_samples"][1] == -1 and np.all(got["state_hits"][1] == -1)
    assert np.isnan(got["probability"][1]) and np.isnan(got["clearance"][1]).all() and np.all(got["worst"][1] == -1)
    assert np.isnan(got["state_clearance"][1]).all() and np.isnan(got["conf"][1]).all()
    _same_bits(got, good, OUT + ("conf",), rows_a=[0, 2], rows_b=[0, 2], what="ok = 0")
    # gpmp2mi_select_best never picks a NaN clearance: probability of a bad row cannot win either way
    best, n = engine.select_best(np.array([3.0, 1.0, 2.0]), None, -got["probability"], required_clearance=-2.0)
    assert (best, n) == (2, 2)


def _refused(engine, p, J, needle):
    r, s = _handles(engine, p)
    pl = engine.plan(r, s, p.setting, p.B)
    try:
        pl.set_problem(*_args(p), p.init)
        fake = 8        # a device address that is never used: the refusal comes first
        for call in (lambda: pl.collision_probability(J, 4, 1), lambda: pl.sample_dense_seeded(J, 4, 1),
                     lambda: pl.collision_probability_dev(J, 4, 1, hits=fake, clearance=fake),
                     lambda: pl.sample_dense_seeded_dev(J, 4, 1, fake)):
            with pytest.raises(E.Gpmp2miError) as ei:
                call()
            assert ei.value.code == 4 and needle in str(ei.value), str(ei.value)
        pl.optimize()                      # the plan is as usable as before
        assert pl.result()["traj"].shape == p.init.shape
    finally:
        pl.close()


def test_wide_plans_are_refused_with_the_limit_named(engine):
    from test_gpu_step_backward_error import _wide
    _refused(engine, _wide(8, 10), 2, "2 dof <= 15")


def test_pose2_plans_are_refused_with_the_missing_piece_named(engine):
    _refused(engine, problems.mobile_arm_config5(), 2, "bridge in the tangent space")


def test_inter_step_64_is_refused_with_the_limit_named(engine):
    _refused(engine, cases.wam(2), 64, "inter_step <= 63")


def test_the_optimizer_is_left_alone(engine):
    p = cases.wam(16)
    pl, r, s = _solved_plan(engine, p)
    twin, _, _ = _solved_plan(engine, p)
    try:
        pl.collision_probability(3, 17, 5, ref.T_MAP)
        pl.sample_dense_seeded(3, 17, 5)
        pl.update(1)
        twin.update(1)
        x, y = pl.result(), twin.result()
    finally:
        pl.close()
        twin.close()
    for name in ("traj", "final_error", "iters", "status"):
        assert np.array_equal(x[name], y[name]), name
