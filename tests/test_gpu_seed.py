"""Seeding on the GPU (include/gpmp2mi.h "seeding"; gpmp2_amd/csrc/seed_kernels.hip, host/seed.hip): the counter RNG
against its numpy restatement (tests/rng_reference.py), the prior precision H_seed against the oracle's linearization over
an obstacle-free field, the restarts against the long-double recursion of tests/posterior_reference.py, and the seeded
queue / posterior against their unseeded siblings fed the same numbers.

Bounds.  All three measured constants come from one run of scripts/seed_error.py over the cases of this file
(profiles/seed_error.txt states the rules and the run):
  normals   |z_gpu - z_numpy| <= Z_TOL: the next power of two above 4 x the largest difference, capped at 1e-12 (the cap
            is a condition: a single-precision log or sincos gives 1e-7 and must not pass).
  H_seed    worst |H - H_oracle| / max |block| <= H_TOL: the next power of two above 4 x the measured value, capped at
            1e-10 (both sides build the same formula from the same fp64 inputs).
  restarts  the measure and rule of tests/test_gpu_posterior.py, e_gpu <= min(max(K e_cpu, FLOOR), 1e-9) on the sigma
            scale, with e_gpu = max |init - (mean + scale truth)| / (scale sigma) -- which is |(init - mean) / scale - truth|
            / sigma -- and e_cpu the larger of that file's float64 yardstick of H_seed and the same measure of the float64
            evaluation mean + scale * sample(H_seed, z).  K and FLOOR are re-derived for these systems by that file's
            rule (K: next power of two above 4 x the largest e_gpu / e_cpu; FLOOR: 4 x the largest e_gpu among the cases
            whose e_cpu < 1e-15), not copied: H_seed with its tight end priors is conditioned differently.
  posterior the seeded samples against the unseeded kernel's on the same z (the engine's normal_fill): max |difference|
            / sigma <= the restarts' bound at that system's e_cpu.  The two kernels run the same products, so equality
            is expected and printed; the bound is what is asserted.  The seeded samples are also held to the long-double
            truth by test_gpu_posterior's own bound: the chains of a solved WAM plan are the ones that file measured.
"""
from __future__ import annotations

import numpy as np
import pytest

import gpmp2_amd as g
import posterior_reference as ref
import rng_reference as rr
import test_gpu_posterior as TP
from gpmp2_amd import _capi, problems
from gpmp2_amd import engine as E
from gpmp2_amd.settings import TrajOptimizerSetting
from gpmp2_amd.trajutils import initArmTrajStraightLine

pytestmark = pytest.mark.gpu

SEED = 0x5EED2026C0FFEE
Z_CAP, H_CAP, CAP = 1e-12, 1e-10, 1e-9
# one measured run of every case of this file (profiles/seed_error.txt):
Z_TOL = min(2.0 ** -48, Z_CAP)   # largest |difference| 4.44e-16 -> 4 x that = 1.78e-15 -> next power of two above
H_TOL = min(2.0 ** -47, H_CAP)   # largest 1.485e-15 (planar, N = 5) -> 4 x that = 5.9e-15 -> next power of two above
K = 8.0                          # largest e_gpu / e_cpu 1.755 (planar D = 2, N = 17, M = 1) -> 4 x that = 7.02
FLOOR = 0.0                      # no case has e_cpu < 1e-15: the rounding of mean + scale delta keeps it at 1e-13 .. 3e-12
CPU_EXACT = 1e-15

FILL_SHAPES = [(1, 1, 1, 1), (3, 2, 2, 7), (2, 17, 5, 14), (33, 1, 18, 15)]   # (a_count, b_count, nblk, n)
NS = (1, 2, 5, 17)
MS = (1, 16, 17, 33)             # one column, a full tile, one past it, two tiles and one


def bound(e_cpu):
    return min(max(K * e_cpu, FLOOR), CAP)


# ---------------------------------------------------------------------------------------------- 1. normals
def measure_fill(engine):
    """-> rows dict(id, diff): largest |normal_fill - restatement| of every shape; asserts finiteness and the sub-range"""
    rows = []
    for stream, (ac, bc, nblk, n) in zip((_capi.RNG_RESTARTS, _capi.RNG_POSTERIOR, 7, 0xABCDEF), FILL_SHAPES):
        a0, b0 = 5 + ac, 1000003 * bc
        got = engine.normal_fill(SEED, stream, a0, ac, b0, bc, nblk, n)
        want = rr.normal_fill(SEED, stream, a0, ac, b0, bc, nblk, n)
        assert got.shape == want.shape and np.all(np.isfinite(got))
        if ac > 1:    # a sub-range is the same function of the same indices
            one = engine.normal_fill(SEED, stream, a0 + 1, 1, b0, bc, nblk, n)
            assert np.array_equal(one[0], got[1])
        rows.append(dict(id=f"normal_fill {ac}x{bc}x{nblk}x{n} stream {stream}", diff=float(np.abs(got - want).max())))
    return rows


def test_normal_fill_against_the_restatement(engine):
    rows = measure_fill(engine)
    for r in rows:
        print(f"{r['id']}: largest |difference| {r['diff']:.2e}, bound {Z_TOL:.2e}")
    for r in rows:
        assert r["diff"] <= Z_TOL, r


# ---------------------------------------------------------------------------------------------- problems
def _free_field(dim):
    """the constant-1000 field: every obstacle factor is zero with a zero Jacobian"""
    return [-2.0] * dim, 0.5, np.full((9,) * dim, 1000.0)


def _planar(D, N, Qc=None):
    arm = g.Arm(D, [0.9 / D] * D, [0.0] * D, [0.0] * D)
    model = g.ArmModel(arm, [g.BodySphere(l, 0.05, (-0.45 / D, 0, 0)) for l in range(D)])
    st = TrajOptimizerSetting(D)
    st.set_total_step(N); st.set_total_time(3.0); st.set_obs_check_inter(1); st.set_cost_sigma(0.1); st.set_epsilon(0.2)
    st.set_conf_prior_model(1e-3); st.set_vel_prior_model(1e-3); st.set_max_iter(4)
    st.set_Qc_model(np.eye(D) if Qc is None else Qc)
    return model, st, 2


def _wam(N):
    return g.generateArm("WAMArm"), problems.wam_setting(N, 1, "GN", 4), 3


def _spd(D):
    A = np.random.default_rng(77).normal(size=(D, D))
    return A @ A.T + D * np.eye(D)


PRIOR_CASES = ([(f"planar D={D} N={N}", lambda D=D, N=N: _planar(D, N)) for D in (1, 2, 4) for N in NS]
               + [(f"WAM N={N}", lambda N=N: _wam(N)) for N in NS]
               + [("planar D=4 N=5 dense Qc", lambda: _planar(4, 5, _spd(4)))])


def _ends(D, M, first=0):
    """start / end configurations of problems first .. first + M - 1: a function of the problem index"""
    j = (first + np.arange(M))[:, None]
    k = np.arange(D)[None, :]
    return 0.1 + 0.01 * j + 0.2 * k, 0.9 - 0.02 * j + 0.05 * k * k


def _plan(engine, make, B=2):
    model, st, dim = make()
    origin, cell, data = _free_field(dim)
    r, s = engine.robot(model), engine.sdf(origin, cell, data)
    return engine.plan(r, s, st, B), model, st, (origin, cell, data), (r, s)


# ---------------------------------------------------------------------------------------------- 2. H_seed
def measure_prior(engine, oracle, cid, make):
    """-> (row dict(id, err), Hd, Ho): H_seed as the plan built it against the oracle's linearization of the same setting"""
    pl, model, st, (origin, cell, data), _ = _plan(engine, make, B=1)
    try:
        Hd, Ho = pl.seed_prior()
    finally:
        pl.close()
    D, N = st.dof, st.total_step
    sc, ec = _ends(D, 1)
    z = np.zeros((1, D))
    init = initArmTrajStraightLine(sc[0], ec[0], N)[None]
    ro, so = oracle.robot(model), oracle.sdf(origin, cell, data)
    Od, Oo, _, _ = oracle.linearize(ro, so, st, sc, z, ec, z, init)
    err = 0.0
    for got, want in ((Hd, Od[0]), (Ho, Oo[0])):
        for i in range(want.shape[0]):
            err = max(err, float(np.abs(got[i] - want[i]).max() / np.abs(want[i]).max()))
    return dict(id=cid, err=err), Hd, Ho


@pytest.mark.parametrize("cid,make", PRIOR_CASES, ids=[c for c, _ in PRIOR_CASES])
def test_seed_prior_against_the_oracle(engine, oracle, cid, make):
    row, Hd, Ho = measure_prior(engine, oracle, cid, make)
    print(f"{cid}: worst |H - H_oracle| / max |block| = {row['err']:.2e}, bound {H_TOL:.2e}")
    assert row["err"] <= H_TOL, row


# ---------------------------------------------------------------------------------------------- 3. restarts
def measure_restarts(engine, cid, make):
    """every M of MS, mean given and NULL, against the long-double recursion on H_seed -> rows dict(id, e_gpu, e_cpu)"""
    pl, model, st, _, _ = _plan(engine, make)
    rows = []
    try:
        D, N = st.dof, st.total_step
        n, nb = 2 * D, N + 1
        Hd, Ho = pl.seed_prior()
        tr = ref.truth(Hd, Ho)
        yard = ref.cpu_yardstick(Hd, Ho, tr)
        sg = ref.sigma_of(tr[0])[None]
        for M in MS:
            first, scale = 3 + M, 0.75
            z = engine.normal_fill(SEED, _capi.RNG_RESTARTS, first, M, 0, 1, nb, n)[:, 0]
            assert np.abs(z - rr.normal_fill(SEED, rr.RESTARTS, first, M, 0, 1, nb, n)[:, 0]).max() <= Z_TOL
            d = ref.truth_sample(Hd, Ho, z)
            d64 = ref.sample(Hd, Ho, z)
            sc, ec = _ends(D, M, first)
            line = np.stack([initArmTrajStraightLine(sc[m], ec[m], N) for m in range(M)])
            given = line + 0.3 * np.sin(np.arange(nb) * 0.7)[None, :, None] * np.cos(np.arange(n))[None, None, :]
            for name, mean, got in (("mean", given, pl.seed_restarts(M, SEED, mean=given, first=first, scale=scale)),
                                    ("line", line, pl.seed_restarts(M, SEED, sc, ec, first=first, scale=scale))):
                LD = ref.LD
                want = mean.astype(LD) + LD(scale) * d
                e_gpu = float((np.abs(got.astype(LD) - want) / (LD(scale) * sg)).max())
                e_cpu = max(yard, float((np.abs((mean + scale * d64).astype(LD) - want) / (LD(scale) * sg)).max()))
                rows.append(dict(id=f"{cid} M={M} {name}", e_gpu=e_gpu, e_cpu=e_cpu))
    finally:
        pl.close()
    return rows


@pytest.mark.parametrize("cid,make", PRIOR_CASES, ids=[c for c, _ in PRIOR_CASES])
def test_restarts_against_the_long_double_recursion(engine, cid, make):
    rows = measure_restarts(engine, cid, make)
    for r in rows:
        print(f"{r['id']}: e_gpu {r['e_gpu']:.2e}, e_cpu {r['e_cpu']:.2e}, bound {bound(r['e_cpu']):.2e}")
    for r in rows:
        assert r["e_gpu"] <= bound(r["e_cpu"]), r


# ---------------------------------------------------------------------------------------------- 4, 5. exactness, indices
@pytest.fixture(scope="module")
def wam17(engine):
    pl, model, st, _, keep = _plan(engine, lambda: _wam(17), B=4)
    yield pl, st
    pl.close()


def test_straight_line_and_zero_scale_are_exact(wam17):
    pl, st = wam17
    D, N, M = st.dof, st.total_step, 19
    sc, ec = _ends(D, M)
    line = np.stack([initArmTrajStraightLine(sc[m], ec[m], N) for m in range(M)])
    got = pl.seed_restarts(M, SEED, sc, ec, keep_first=True)
    assert np.array_equal(got[0], line[0])
    assert not np.array_equal(got[1], line[1])
    assert np.array_equal(pl.seed_restarts(M, SEED, sc, ec, scale=0.0), line)
    mean = np.random.default_rng(3).normal(size=line.shape)
    assert np.array_equal(pl.seed_restarts(M, SEED, mean=mean, scale=0.0), mean)
    # keep_first holds problem 0, not row 0
    moved = pl.seed_restarts(M, SEED, sc, ec, first=1, keep_first=True)
    assert not np.array_equal(moved[0], line[0])


def test_a_problem_depends_on_its_index_alone(engine, wam17):
    pl, st = wam17
    D, N, M = st.dof, st.total_step, 40
    sc, ec = _ends(D, M)
    whole = pl.seed_restarts(M, SEED, sc, ec, scale=0.5)
    a = pl.seed_restarts(17, SEED, sc[:17], ec[:17], first=0, scale=0.5)
    b = pl.seed_restarts(23, SEED, sc[17:], ec[17:], first=17, scale=0.5)
    assert np.array_equal(whole, np.concatenate([a, b]))
    assert np.array_equal(pl.seed_restarts(1, SEED, sc[5:6], ec[5:6], first=5, scale=0.5)[0], whole[5])
    assert not np.array_equal(pl.seed_restarts(1, SEED + 1, sc[5:6], ec[5:6], first=5, scale=0.5)[0], whole[5])
    # the `_dev` form into a caller's buffer
    lib = engine.lib
    import ctypes as C
    bufs = []

    def dev(x):
        p = C.c_void_p()
        assert lib.gpmp2mi_debug_device_alloc(C.c_size_t(x.nbytes), 0, C.byref(p)) == 0
        assert lib.gpmp2mi_debug_device_write(p, x.ctypes.data_as(C.c_void_p), C.c_size_t(x.nbytes)) == 0
        bufs.append(p)
        return p.value

    try:
        out = np.zeros_like(whole)
        d_out = dev(out)
        pl.seed_restarts_dev(M, SEED, d_out, dev(sc), dev(ec), scale=0.5)
        assert lib.gpmp2mi_debug_device_read(out.ctypes.data_as(C.c_void_p), C.c_void_p(d_out), C.c_size_t(out.nbytes)) == 0
        assert np.array_equal(out, whole)
    finally:
        for p in bufs:
            lib.gpmp2mi_debug_device_free(p)


# ---------------------------------------------------------------------------------------------- 6. queue
@pytest.mark.parametrize("opt", ["GN", "LM"])
def test_seeded_queue_equals_seed_then_queue(engine, opt):
    p = problems.wam_restarts(B=16, total_step=17, obs_check_inter=2, opt=opt, sdf="40", max_iter=12)
    M, D = 40, 7
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    sc, ec = np.repeat(p.start_conf[:1], M, 0), np.repeat(p.end_conf[:1], M, 0)
    zv = np.zeros((M, D))
    kw = dict(first=2, scale=0.4, keep_first=True)
    pl = engine.plan(r, s, p.setting, 16)
    try:
        init = pl.seed_restarts(M, SEED, sc, ec, **kw)
        want = pl.optimize_queue(sc, zv, ec, zv, init)
        got = pl.optimize_queue_seeded(SEED, sc, zv, ec, zv, want_init=True, **kw)
    finally:
        pl.close()
    assert np.array_equal(got["init"], init)
    for name in ("iters", "status", "final_error", "error_trace", "traj"):    # unused trace entries are NaN in both
        assert np.array_equal(got[name], want[name], equal_nan=name == "error_trace"), name
    mp = engine.multi_plan(r, s, p.setting, 16, [0, 0])
    try:
        multi = mp.optimize_queue_seeded(SEED, sc, zv, ec, zv, want_init=True, **kw)
    finally:
        mp.close()
    for name in ("init", "iters", "status", "final_error", "error_trace", "traj"):
        assert np.array_equal(multi[name], got[name], equal_nan=name == "error_trace"), f"multi plan: {name}"


# ---------------------------------------------------------------------------------------------- 7. posterior
def measure_posterior(engine, N):
    """WAM, B = 3, solved; K of (1, 16, 17): the seeded samples against the truth on the engine's own linearization at
    the result, and against the unseeded kernel fed the same z (e_same, sigma scale) -> rows dict(id, e_gpu, e_cpu,
    e_plain, e_same, same); asserts ok, the untouched optimizer and the sample index"""
    p = problems.wam_restarts(B=3, total_step=N, obs_check_inter=2, opt="GN", sdf="40")
    args = (p.start_conf, p.start_vel, p.end_conf, p.end_vel)
    r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
    pl, twin = engine.plan(r, s, p.setting, 3), engine.plan(r, s, p.setting, 3)
    rows = []
    try:
        for q in (pl, twin):
            q.set_problem(*args, p.init)
            q.optimize()
        traj = pl.result()["traj"]
        Hd, Ho, _, _ = pl.linearize(traj)
        n, nb, row_first, sample_first = 14, N + 1, 11, 5
        Sd = [ref.truth(Hd[b], Ho[b])[0] for b in range(3)]
        for Ks in (1, 16, 17):
            delta, ok = pl.sample_posterior_seeded(Ks, SEED, row_first, sample_first)
            assert list(ok) == [1, 1, 1]
            z = engine.normal_fill(SEED, _capi.RNG_POSTERIOR, row_first, 3, sample_first, Ks, nb, n)
            plain = pl.sample_posterior(z)
            row = TP._sample_row(f"WAM N={N} seeded posterior K={Ks}", Hd, Ho, z, delta)
            row["same"] = bool(np.array_equal(delta, plain))
            row["e_same"] = max(ref.sample_error(delta[b], plain[b], Sd[b]) for b in range(3))
            row["e_plain"] = TP._sample_row("", Hd, Ho, z, plain)["e_gpu"]
            rows.append(row)
            if Ks == 17:    # a sample is a function of its index, not of the tile it rides in
                one, _ = pl.sample_posterior_seeded(1, SEED, row_first, sample_first + 16)
                assert np.array_equal(one[:, 0], delta[:, 16])
        pl.update(1)
        twin.update(1)
        assert np.array_equal(pl.result()["traj"], twin.result()["traj"]), "the seeded posterior touched the optimizer"
    finally:
        pl.close()
        twin.close()
    return rows


@pytest.mark.parametrize("N", [1, 5, 16])
def test_seeded_posterior_equals_the_unseeded_one(engine, N):
    rows = measure_posterior(engine, N)
    for r in rows:
        print(f"{r['id']}: seeded - unseeded on the same z {r['e_same']:.2e} (bit-identical: {r['same']}), bound "
              f"{bound(r['e_cpu']):.2e}; against the truth: e_gpu {r['e_gpu']:.2e} (unseeded: {r['e_plain']:.2e}), e_cpu "
              f"{r['e_cpu']:.2e}, bound {TP.bound(r['e_cpu']):.2e}")
    for r in rows:
        assert r["e_same"] <= bound(r["e_cpu"]), r       # the two kernels, by the rule of the restarts above
        assert r["e_gpu"] <= TP.bound(r["e_cpu"]), r     # and the seeded one against the truth


# ---------------------------------------------------------------------------------------------- 8. refusals
def test_refusals(engine):
    from test_gpu_step_backward_error import _wide
    for make, word in ((lambda: _wide(8, 10), "dof <= 7"), (problems.mobile_arm_config5, "Pose2")):
        p = make()
        r, s = engine.robot(p.model), engine.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
        pl = engine.plan(r, s, p.setting, p.B)
        try:
            D = p.setting.dof
            zv = np.zeros((p.B, D))
            calls = [lambda: pl.seed_restarts(p.B, SEED, p.start_conf, p.end_conf),
                     lambda: pl.optimize_queue_seeded(SEED, p.start_conf, zv, p.end_conf, zv),
                     lambda: pl.seed_prior()]
            pl.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
            calls.append(lambda: pl.sample_posterior_seeded(2, SEED))
            for call in calls:
                with pytest.raises(E.Gpmp2miError) as ei:
                    call()
                assert ei.value.code == 4 and word in str(ei.value), str(ei.value)
            pl.optimize()      # the plan is as usable as before
            assert np.all(np.isfinite(pl.result()["final_error"]))
        finally:
            pl.close()


def test_bad_arguments_are_invalid(engine, wam17):
    pl, st = wam17
    D, N = st.dof, st.total_step
    sc, ec = _ends(D, 4)
    lib, h = engine.lib, pl.h.ptr
    out = np.zeros((4, N + 1, 2 * D))
    a = (E.dptr(sc), E.dptr(ec), None, E.dptr(out))
    assert lib.gpmp2mi_plan_seed_restarts(h, 0, SEED, 0, 1.0, 0, *a) == 1
    assert lib.gpmp2mi_plan_seed_restarts(h, 4, SEED, -1, 1.0, 0, *a) == 1
    assert lib.gpmp2mi_plan_seed_restarts(h, 4, SEED, 0, -1.0, 0, *a) == 1
    assert lib.gpmp2mi_plan_seed_restarts(h, 4, SEED, 0, float("nan"), 0, *a) == 1
    assert lib.gpmp2mi_plan_seed_restarts(h, 4, SEED, 0, float("inf"), 0, *a) == 1
    assert lib.gpmp2mi_plan_seed_restarts(h, 4, SEED, 0, 1.0, 0, None, E.dptr(ec), None, E.dptr(out)) == 1
    assert lib.gpmp2mi_plan_seed_restarts(h, 4, SEED, 0, 1.0, 0, E.dptr(sc), E.dptr(ec), None, None) == 1
    assert lib.gpmp2mi_plan_seed_restarts(None, 4, SEED, 0, 1.0, 0, *a) == 1
    z = E.dptr(np.zeros((4, D)))
    assert lib.gpmp2mi_plan_optimize_queue_seeded(h, 4, SEED, 0, 1.0, 0, E.dptr(sc), None, E.dptr(ec), z, None, None,
                                                  None, None, None, None, None) == 1
    assert lib.gpmp2mi_plan_optimize_queue_seeded(h, 0, SEED, 0, 1.0, 0, E.dptr(sc), z, E.dptr(ec), z, None, None,
                                                  None, None, None, None, None) == 1
    fresh, _, _, _, _ = _plan(engine, lambda: _wam(2))
    try:
        d = np.zeros((2, 1, 3, 14))
        assert lib.gpmp2mi_plan_sample_posterior_seeded(fresh.h.ptr, 1, SEED, 0, 0, E.dptr(d), None) == 1
        assert b"set_problem" in lib.gpmp2mi_last_error()
        assert lib.gpmp2mi_plan_sample_posterior_seeded(fresh.h.ptr, 0, SEED, 0, 0, E.dptr(d), None) == 1
        assert lib.gpmp2mi_plan_sample_posterior_seeded(fresh.h.ptr, 1, SEED, 0, 0, None, None) == 1
    finally:
        fresh.close()
    one = np.zeros(4)
    assert lib.gpmp2mi_normal_fill(SEED, 1, 0, 1, 0, 1, 1, 17, E.dptr(np.zeros(17))) == 1
    assert lib.gpmp2mi_normal_fill(SEED, 1, -1, 1, 0, 1, 1, 4, E.dptr(one)) == 1
    assert lib.gpmp2mi_normal_fill(SEED, 1 << 24, 0, 1, 0, 1, 1, 4, E.dptr(one)) == 1
    assert lib.gpmp2mi_normal_fill(SEED, 1, 0, 1, 0, 1, 1, 4, None) == 1
    # and the plan seeds normally afterwards
    assert np.all(np.isfinite(pl.seed_restarts(4, SEED, sc, ec)))
