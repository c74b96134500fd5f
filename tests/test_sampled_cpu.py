"""Pins the definitions and the yardstick of tests/sampled_reference.py on the CPU oracle (no GPU needed), the conditions
the cases of tests/test_gpu_sampled.py must meet, and the entry points of the sampled clearance (include/gpmp2mi.h) as
far as they go without a device.

Measured here on the oracle-solved WAM problems of tests/test_risk_cpu.py (sdf "40", B = 3) at (N, J) = (5, 5), (16, 3),
(33, 1) with K = 256: the float64 spread of the reference (support samples from float64 against long double) stays below
1e-12 on both maps; a relative slip of 1e-6 in one entry of the bridge factor or in the support samples moves a sampled
configuration and a per-state clearance by more than CAP = 1e-9, while the row minimum c_s of the rows that attain it at a
support state does not move at all under the slips of the bridge factor.  So the GPU bound is gated on the maps.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import posterior_reference as post
import risk_reference as risk
import sampled_cases as cases
import sampled_reference as ref
import score_reference as sref
from test_risk_cpu import solved

CAP = ref.CAP
LD = ref.LD


# ---------------------------------------------------------------------------------------------- 1. the bridge formula
@pytest.mark.parametrize("dt", [0.1, 0.5, 2.0])
def test_closed_bridge_covariance_equals_the_kernel_form(dt):
    for J in (1, 2, 5, 9, 63):
        a, b = ref.bridge_closed(dt, J), ref.bridge_from_kernel(dt, J)
        scale = np.sqrt(np.outer(np.diag(a), np.diag(a)))
        e = float((np.abs(a - b) / scale).max())
        # long double (eps 1.1e-19) times the cancellation of the subtractive form: near the end of the interval the
        # result is (D - t)^3 / D^3 >= (J + 1)^-3 of its terms.  Measured 4.2e-14 at J = 63, 7.5e-17 at J = 9.
        assert e < 8 * float(np.finfo(LD).eps) * (J + 1) ** 3, (dt, J, e)
        for j in range(1, J + 1):
            tau = LD(j) * (LD(dt) / LD(J + 1))
            # at s = t the last factor is 2 t (D - t), formed from terms of size t D: a cancellation of at most J + 1
            assert abs(a[j - 1, j - 1] - risk.qc_closed(dt, tau)[0, 0]) <= 8 * (J + 1) * np.finfo(LD).eps * a[j - 1, j - 1], (dt, J, j)
        assert np.array_equal(a, a.T) and np.all(np.linalg.eigvalsh(a.astype(np.float64)) > 0), (dt, J)
        L = ref.chol_lower(a.astype(np.float64), np.float64)
        res = float((np.abs(L @ L.T - a.astype(np.float64)) / scale.astype(np.float64)).max())
        print(f"dt={dt} J={J}: closed against kernel form {e:.1e}, cond {np.linalg.cond(a.astype(np.float64)):.1e}, "
              f"fp64 Cholesky residual {res:.1e}")
        assert res < 4e-16 * J, (dt, J, res)


# ---------------------------------------------------------------------------------------------- 2. the joint law
def test_the_joint_law_is_that_of_the_fine_chain():
    """the fine-chain construction of test_dense_formula_equals_the_fine_chain_inverse (D = 2, non-diagonal Qc, N = 3,
    J = 2): the covariance the definitions imply for (x(m), x(m')) -- the support covariance through the interpolation,
    plus (Lp Lp^T)[a][b] Qc inside one interval -- equals the configuration blocks of the dense inverse, off-diagonal
    ones inside and across intervals included"""
    rng = np.random.default_rng(21)
    D, N, J, dt = 2, 3, 2, 0.4
    n, Md, h = 2 * D, N * (J + 1) + 1, dt / (J + 1)
    A = rng.normal(size=(D, D))
    Qc = A @ A.T + 0.5 * np.eye(D)
    I = np.eye(D)
    Phi = np.kron(np.array([[1, h], [0, 1.0]]), I)
    Qinv = np.linalg.inv(np.kron(np.array([[h ** 3 / 3, h ** 2 / 2], [h ** 2 / 2, h]]), Qc))
    H = np.zeros((Md * n, Md * n))
    blk = lambda a, b: (slice(a * n, (a + 1) * n), slice(b * n, (b + 1) * n))
    for k in range(Md - 1):                                   # z_{k+1} - Phi z_k ~ N(0, Q(h) (x) Qc)
        H[blk(k, k)] += Phi.T @ Qinv @ Phi
        H[blk(k + 1, k + 1)] += Qinv
        H[blk(k, k + 1)] -= Phi.T @ Qinv
        H[blk(k + 1, k)] -= Qinv @ Phi
    for i in range(N + 1):                                    # information on the support states
        M = rng.normal(size=(n, n))
        H[blk(i * (J + 1), i * (J + 1))] += M @ M.T + 0.1 * np.eye(n)
    L2, P2 = risk.gp_scalars(dt, 2 * h, np.float64)           # a likelihood on a . (Lambda z_1 + Psi z_2)
    a = rng.normal(size=(1, n))
    row = np.zeros((1, Md * n))
    row[:, blk(1 * (J + 1), 0)[0]] = a @ np.kron(L2, I)
    row[:, blk(2 * (J + 1), 0)[0]] = a @ np.kron(P2, I)
    H += row.T @ row / 0.05 ** 2
    S = np.linalg.inv(H)
    sup = np.concatenate([np.arange(i * (J + 1) * n, i * (J + 1) * n + n) for i in range(N + 1)])
    S_sup = S[np.ix_(sup, sup)]                               # the law of the support samples: the whole of it
    T = np.zeros((Md * D, (N + 1) * n))                       # x(m) = T [z_0 .. z_N] + eps(m)
    bridge = np.zeros((Md * D, Md * D))
    Pb = ref.bridge_closed(dt, J, np.float64)
    for m in range(Md):
        i, j = divmod(m, J + 1)
        if j == 0:
            T[m * D:(m + 1) * D, i * n:i * n + D] = I
            continue
        Lm, Pm = risk.gp_scalars(dt, j * h, np.float64)
        T[m * D:(m + 1) * D, i * n:(i + 1) * n] = np.kron(Lm[0:1], I)
        T[m * D:(m + 1) * D, (i + 1) * n:(i + 2) * n] = np.kron(Pm[0:1], I)
        for jb in range(1, J + 1):
            mb = i * (J + 1) + jb
            bridge[m * D:(m + 1) * D, mb * D:(mb + 1) * D] = Pb[j - 1, jb - 1] * Qc
    implied = T @ S_sup @ T.T + bridge
    xs = np.concatenate([np.arange(m * n, m * n + D) for m in range(Md)])
    truth = S[np.ix_(xs, xs)]
    sg = np.sqrt(np.diag(truth))
    e = float((np.abs(implied - truth) / np.outer(sg, sg)).max())
    print(f"joint law against the fine-chain inverse: {e:.2e}")
    assert e < 1e-12                                          # as the dense formula: 100 x for the conditioning of the inverse
    # ... and the factor reproduces the bridge part: Lp Lp^T = P
    Lp = ref.bridge_factor(dt, J)
    assert float(np.abs(Lp @ Lp.T - ref.bridge_closed(dt, J)).max()) < 1e-20


# ---------------------------------------------------------------------------------------------- 3. yardstick and CAP
def _solved_row(oracle, c, b, J, K, dtype=np.float64, bridge=True, Lp=None, scale=None, seed=cases.SEED):
    p = c["p"]
    ro, fld = oracle.robot(p.model), sref.oracle_sdf(oracle, p.sdf_origin, p.sdf_cell, p.sdf_data)
    delta = ref.support_samples(c["Hd"][b], c["Ho"][b], seed, b, 0, K, dtype)
    if scale is not None:
        delta = delta * scale
    return ref.row(oracle, ro, fld, c["radius"], p.setting.Qc, c["D"], c["dt"], J, c["traj"][b], delta, seed, b, 0, bridge, Lp)


def _moved(a, b):
    fin = np.isfinite(a["state"]) & np.isfinite(b["state"])
    return (float(np.abs(a["conf"] - b["conf"]).max()), float(np.abs(a["state"][fin] - b["state"][fin]).max()),
            float(np.abs(a["clearance"] - b["clearance"]).max()))


@pytest.mark.parametrize("N,J", [(5, 5), (16, 3), (33, 1)])
def test_float64_spread_stays_below_cap_and_the_slips_do_not(oracle, N, J):
    c, K = solved(oracle, N, J), 256
    Lp = ref.bridge_factor(c["dt"], J)
    blind = 0
    for b in range(3):
        base = _solved_row(oracle, c, b, J, K)
        sp = _moved(base, _solved_row(oracle, c, b, J, K, LD))
        print(f"N={N} J={J} row {b}: float64 spread conf {sp[0]:.1e}, state_clearance {sp[1]:.1e}")
        assert sp[0] < CAP and sp[1] < CAP
        slips = [("Lp[J-1][J-1]", (J - 1, J - 1))] + ([("Lp[1][0]", (1, 0))] if J >= 2 else [])
        for name, at in slips:
            L = Lp.copy()
            L[at] *= 1 + LD(1e-6)
            mv = _moved(base, _solved_row(oracle, c, b, J, K, Lp=L))
            print(f"    1e-6 slip in {name}: conf {mv[0]:.1e}, state_clearance {mv[1]:.1e}, c_s {mv[2]:.1e}")
            assert mv[0] > CAP and mv[1] > CAP, (N, J, b, name)
            # a row whose every sample attains its minimum at a support state is blind to the bridge factor
            if np.all(base["worst"][:, 0] % (J + 1) == 0):
                assert mv[2] == 0.0, (N, J, b, name, mv[2])
                blind += 1
        mv = _moved(base, _solved_row(oracle, c, b, J, K, scale=1 + 1e-6))
        print(f"    1e-6 slip in delta: conf {mv[0]:.1e}, state_clearance {mv[1]:.1e}, c_s {mv[2]:.1e}")
        assert mv[0] > CAP and mv[1] > CAP, (N, J, b, "delta")
    assert blind >= 1, "no row shows that c_s alone misses a slip of the bridge factor"


def test_without_the_bridge_the_samples_are_visibly_different(oracle):
    c = solved(oracle, 5, 5)
    mv = _moved(_solved_row(oracle, c, 0, 5, 64), _solved_row(oracle, c, 0, 5, 64, bridge=False))
    print(f"dropping the bridge noise: conf {mv[0]:.1e} rad, state_clearance {mv[1]:.1e} m")
    assert mv[0] > 1e-2 and mv[1] > 1e-3


# ---------------------------------------------------------------------------------------------- 4. the GPU cases
@pytest.mark.parametrize("robot", cases.ROBOTS + ("arm3", "arm5", "arm6"))
def test_thresholds_of_the_gpu_cases_leave_nothing_undecided(oracle, robot):
    """conditions on the inputs of tests/test_gpu_sampled.py, not measurements: at the seed and K it uses, no reference
    value lies within CAP of a threshold (T_med of each row, T_map = 0.08), hits / K at T_med lies in [0.1, 0.9], and T_map
    leaves at least 3 checked states of some row with a state_hits strictly between 0 and K -- in every case but (1, 0),
    which has two checked states, both pinned.  A case that breaks them gets another seed or goal in sampled_cases.py
    (the resting rows at N = 1, the seed of the point robot at (5, 5)), not a wider cap."""
    K = cases.K_REF
    for N, J in [(n, j) for r, n, j in cases.ALL if r == robot]:
        c = cases.ctx(oracle, robot, N, J)
        mixed = 0
        for bridge in (0, 1):
            for b in range(cases.B):
                r = c.row(b, bridge)
                T = ref.t_med(r["clearance"])
                for thr in (T, ref.T_MAP):
                    assert ref.counts(r["state"], thr, CAP)["undecided"] == 0, (robot, N, J, bridge, b, thr)
                assert 0.1 <= ref.counts(r["state"], T)["hits"] / K <= 0.9, (robot, N, J, bridge, b)
                sh = ref.counts(r["state"], ref.T_MAP)["state_hits"]
                if bridge:
                    mixed = max(mixed, int(((sh > 0) & (sh < K)).sum()))
        print(f"{robot} N={N} J={J}: {mixed} checked states of the best row with 0 < state_hits < K at T_map")
        if (N, J) != (1, 0):
            assert mixed >= 3, (robot, N, J, mixed)


# ---------------------------------------------------------------------------------------------- 5. statistics
def test_the_references_own_samples_have_the_moments_of_the_dense_marginals(oracle):
    """WAM (5, 5), row 0, K = 4 096: what tests/test_gpu_sampled.py asks of the device's samples, asked of the
    reference's first -- and without the bridge the variance in the middle of an interval is too small"""
    from test_gpu_sampled import statistics_bounds
    c, J, K, b = solved(oracle, 5, 5), 5, 4096, 0
    D, Qc = c["D"], c["p"].setting.Qc
    delta = ref.support_samples(c["Hd"][b], c["Ho"][b], 4242, b, 0, K)
    eps = ref.bridge_noise(Qc, D, c["dt"], J, 5, 4242, b, 0, K)
    plain = ref.configurations(oracle, D, c["dt"], J, c["traj"][b], delta).astype(np.float64)
    conf = (plain + eps).astype(np.float64)
    cov = risk.dense_cov(*post.truth(c["Hd"][b], c["Ho"][b]), Qc, c["dt"], J).astype(np.float64)
    var = np.diagonal(cov[:, :D, :D], axis1=1, axis2=2)
    mean = oracle.interpolate_traj(D, 0, None, c["dt"], J, c["traj"][b][None])[0][:, :D]
    zm, zv = statistics_bounds(conf, mean, var, K)
    print(f"with the bridge: mean {zm.max():.2f} sigma / sqrt K, variance {zv.max():.2f} sqrt(2 / K)")
    assert zm.max() < 5 and zv.max() < 5
    _, zv0 = statistics_bounds(plain, mean, var, K)
    mid = np.arange(conf.shape[1]) % (J + 1) == (J + 1) // 2
    print(f"without: variance {zv0[mid].max():.2f} sqrt(2 / K) at the mid-interval sub-steps")
    assert zv0[mid].max() > 5


# ---------------------------------------------------------------------------------------------- 6. the C ABI, no device
def _eng():
    from gpmp2_amd import engine
    return engine.Engine()


NAMES = ("gpmp2mi_sampled_clearance_traj", "gpmp2mi_sampled_clearance_traj_dev", "gpmp2mi_plan_collision_probability",
         "gpmp2mi_plan_collision_probability_dev", "gpmp2mi_plan_sample_dense_seeded", "gpmp2mi_plan_sample_dense_seeded_dev",
         "gpmp2mi_debug_sampled_chunk_bytes")


def test_entry_points_have_the_declared_signatures():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "gpmp2mi.h")).read()
    pub = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    outs = ("int* hits, double* probability, double* clearance, int* worst, double* state_clearance, int* state_hits, "
            "int* oor_samples")
    traj = ("(const gpmp2mi_robot* robot, const gpmp2mi_sdf* sdf, const double* Qc, double delta_t, int inter_step, int B, "
            "int total_step, int K, const double* traj, const double* delta, const int* ok, uint64_t seed, int row_first, "
            f"int sample_first, int bridge, double required_clearance, {outs}, double* conf")
    plan = ("(gpmp2mi_plan* p, int inter_step, int K, uint64_t seed, int row_first, int sample_first, int bridge")
    for decl in (
        f"int gpmp2mi_sampled_clearance_traj{traj});",
        f"int gpmp2mi_sampled_clearance_traj_dev{traj}, void* stream);",
        f"int gpmp2mi_plan_collision_probability{plan}, double required_clearance, {outs}, int* ok);",
        f"int gpmp2mi_plan_collision_probability_dev{plan}, double required_clearance, {outs}, int* ok, void* stream);",
        f"int gpmp2mi_plan_sample_dense_seeded{plan}, double* conf, int* ok);",
        f"int gpmp2mi_plan_sample_dense_seeded_dev{plan}, double* conf, int* ok, void* stream);",
        "enum { GPMP2MI_RNG_BRIDGE = 3 };",
    ):
        assert decl in pub, decl
    assert "sampled clearance" in text and "fifth exception" in text
    lib = _eng().lib
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name


def test_bad_arguments_are_refused_before_any_device_work():
    from gpmp2_amd import engine
    lib = _eng().lib
    d = engine.dptr
    t, de = np.zeros((1, 3, 4)), np.zeros((1, 2, 3, 4))
    fake = ctypes.c_void_p(8)          # a handle that is never read: the refusal comes first
    good = dict(dt=0.1, J=2, B=1, N=2, K=2, rf=0, sf=0, T=0.05)

    def call(r=fake, s=fake, traj=t, delta=de, **kw):
        a = dict(good, **kw)
        return lib.gpmp2mi_sampled_clearance_traj(r, s, None, a["dt"], a["J"], a["B"], a["N"], a["K"],
                                                  None if traj is None else d(traj), None if delta is None else d(delta),
                                                  None, 7, a["rf"], a["sf"], 1, a["T"], *[None] * 8)

    assert call(r=None) == 1 and b"null" in lib.gpmp2mi_last_error()
    assert call(s=None) == 1 and call(traj=None) == 1 and call(delta=None) == 1
    assert call(J=-1) == 1 and b"inter_step" in lib.gpmp2mi_last_error()
    assert call(B=-1) == 1 and b"B must" in lib.gpmp2mi_last_error()
    assert call(N=0) == 1 and b"total_step" in lib.gpmp2mi_last_error()
    assert call(dt=0.0) == 1 and call(dt=-1.0) == 1 and b"delta_t" in lib.gpmp2mi_last_error()
    assert call(K=0) == 1 and b"K must" in lib.gpmp2mi_last_error()
    assert call(rf=-1) == 1 and call(sf=-1) == 1 and b"sample_first" in lib.gpmp2mi_last_error()
    assert call(sf=2 ** 31 - 2, K=2) == 1 and call(rf=2 ** 31 - 1) == 1            # first + count overflows an int
    assert call(T=float("nan")) == 1 and b"required_clearance" in lib.gpmp2mi_last_error()
    assert call(J=64) == 4 and b"inter_step <= 63" in lib.gpmp2mi_last_error()
    assert lib.gpmp2mi_sampled_clearance_traj_dev(None, fake, None, 0.1, 2, 1, 2, 2, 8, 8, None, 7, 0, 0, 1, 0.0,
                                                  *[None] * 9) == 1
    assert lib.gpmp2mi_sampled_clearance_traj_dev(fake, fake, None, 0.1, 2, 1, 2, 0, 8, 8, None, 7, 0, 0, 1, 0.0,
                                                  *[None] * 9) == 1
    # plans
    outs = [None] * 8
    assert lib.gpmp2mi_plan_collision_probability(None, 2, 4, 7, 0, 0, 1, 0.0, *outs) == 1
    assert b"null plan" in lib.gpmp2mi_last_error()
    assert lib.gpmp2mi_plan_collision_probability_dev(None, 2, 4, 7, 0, 0, 1, 0.0, *outs, None) == 1
    assert lib.gpmp2mi_plan_sample_dense_seeded(None, 2, 4, 7, 0, 0, 1, None, None) == 1
    assert lib.gpmp2mi_plan_sample_dense_seeded_dev(None, 2, 4, 7, 0, 0, 1, None, None, None) == 1
    assert lib.gpmp2mi_plan_collision_probability(fake, -1, 4, 7, 0, 0, 1, 0.0, *outs) == 1
    assert b"inter_step" in lib.gpmp2mi_last_error()
    assert lib.gpmp2mi_debug_sampled_chunk_bytes(4096) == 0 and lib.gpmp2mi_debug_sampled_chunk_bytes(0) == 0


def test_without_a_gpu_the_calls_say_so():
    """no quiet fall-back: a robot handle cannot even be made without a device (with one, a tiny call succeeds)"""
    from gpmp2_amd import engine
    eng = _eng()
    p = cases.planar(2)
    if eng.device_count() == 0:
        with pytest.raises(engine.Gpmp2miError) as ei:
            eng.robot(p.model)
        assert ei.value.code == 2
    else:
        r, s = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
        o = eng.sampled_clearance_traj(r, s, None, 0.2, 1, p.init, np.zeros((3, 2, 3, 4)), 1, 0.0)
        assert o["clearance"].shape == (3, 2) and np.isfinite(o["clearance"]).all()


def test_wrappers_reject_bad_shapes_before_the_library():
    from gpmp2_amd import engine

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError(f"reached the library: {name}")

    class Rob:
        dof, S, ptr = 3, 4, None

    eng = engine.Engine.__new__(engine.Engine)
    eng.lib = NoLib()
    traj, delta = np.zeros((2, 5, 6)), np.zeros((2, 4, 5, 6))
    call = lambda **kw: eng.sampled_clearance_traj(Rob(), Rob(), kw.pop("Qc", None), kw.pop("dt", 0.1), kw.pop("J", 2),
                                                   kw.pop("traj", traj), kw.pop("delta", delta), 7, **kw)
    with pytest.raises(ValueError, match="traj: expected"):
        call(traj=np.zeros((2, 5, 4)))
    with pytest.raises(ValueError, match="delta: expected"):
        call(delta=np.zeros((2, 4, 4, 6)))
    with pytest.raises(ValueError, match="delta: expected"):
        call(delta=np.zeros((3, 4, 5, 6)))
    with pytest.raises(ValueError, match="Qc: expected"):
        call(Qc=np.eye(2))
    with pytest.raises(ValueError, match="inter_step"):
        call(J=-1)
    with pytest.raises(ValueError, match="delta_t"):
        call(dt=0.0)
    with pytest.raises(ValueError, match="ok: expected"):
        call(ok=np.ones(3))
    with pytest.raises(ValueError, match="required_clearance"):
        call(required_clearance=float("nan"))
    with pytest.raises(ValueError, match="row_first"):
        call(row_first=-1)
    pl = engine.Plan.__new__(engine.Plan)
    pl.eng, pl.B, pl.D, pl.N, pl.h, pl.robot = eng, 2, 3, 4, None, Rob()
    with pytest.raises(ValueError, match="inter_step"):
        pl.collision_probability(-1, 4, 7)
    with pytest.raises(ValueError, match="K must"):
        pl.collision_probability(2, 0, 7)
    with pytest.raises(ValueError, match="required_clearance"):
        pl.collision_probability_dev(2, 4, 7, required_clearance=float("nan"))
    with pytest.raises(ValueError, match="sample_first"):
        pl.sample_dense_seeded(2, 4, 7, sample_first=-1)
    with pytest.raises(ValueError, match="conf is required"):
        pl.sample_dense_seeded_dev(2, 4, 7, None)

    class Tensor:                      # what _dev_arg reads of a torch tensor
        dtype, shape = "torch.float64", (2, 4, 9)

        class device:
            type = "cuda"

        def is_contiguous(self):
            return True

        def data_ptr(self):
            return 8

    with pytest.raises(ValueError, match="state_clearance: expected"):
        pl.collision_probability_dev(2, 4, 7, state_clearance=Tensor())          # Md = 13 for inter_step = 2
    with pytest.raises(ValueError, match="conf: expected"):
        pl.sample_dense_seeded_dev(2, 4, 7, Tensor())
