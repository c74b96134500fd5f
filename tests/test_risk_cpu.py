"""Pins the definitions and the yardstick of tests/risk_reference.py on the CPU oracle (no GPU needed), and checks the
entry points of the posterior on the executed timeline (include/gpmp2mi.h) as far as they go without a device.

Measured here on the WAM (sdf "40", B = 3, obs_check_inter = 2, solved by the oracle) at (N, J) = (1, 5), (5, 5), (16, 3),
(33, 1), against long double: the float64 compositions (block recursion or dense inverse for the band, then the float64
formula) give e_cov <= 1.6e-10 (the dense inverse at N = 33; the recursion <= 2.2e-12) and e_sig <= 2.8e-12; a relative
slip of 1e-6 in Psi_2[0][1] of checked state 1 gives e_cov >= 1.2e-7 and e_sig >= 2.6e-8 for N >= 5 (N = 1 does not see
it: 6e-15).  CAP = 1e-9, the ceiling of the GPU bound (tests/test_gpu_risk.py), therefore lets every float64 yardstick
pass and stops the slip; this file asserts both."""
import ctypes
import os
import re

import numpy as np
import pytest

import posterior_reference as post
import risk_reference as ref
import score_reference as sref
from gpmp2_amd import problems

CAP = 1e-9
LD = ref.LD
_SOLVED = {}


def _args(p):
    return p.start_conf, p.start_vel, p.end_conf, p.end_vel


def solved(oracle, N, J):
    """the WAM problem at N solved by the oracle, with its linearization there and the oracle's geometry of the J-fold
    up-sampled result: computed once per (N, J) and shared"""
    if (N, J) not in _SOLVED:
        p = problems.wam_restarts(B=3, total_step=N, obs_check_inter=2, opt="GN", sdf="40")
        ro, fld = oracle.robot(p.model), sref.oracle_sdf(oracle, p.sdf_origin, p.sdf_cell, p.sdf_data)
        traj = oracle.batch_optimize(ro, fld.handle, p.setting, *_args(p), p.init)["traj"]
        Hd, Ho, _, _ = oracle.linearize(ro, fld.handle, p.setting, *_args(p), traj)
        dt, D = sref.delta_t(p.setting), p.setting.dof
        geo = [ref.geometry(oracle, ro, fld.handle, False, D, dt, J, traj[b], p.sdf_origin, p.sdf_cell) for b in range(p.B)]
        score = sref.oracle_score(oracle, p.model, ro, fld, dt, J, traj)
        _SOLVED[(N, J)] = dict(p=p, traj=traj, Hd=Hd, Ho=Ho, dt=dt, D=D, geo=geo, score=score,
                               radius=np.asarray(p.model.flat()["sphere_radius"], dtype=np.float64))
    return _SOLVED[(N, J)]


# ---------------------------------------------------------------------------------------------- the formula
def test_closed_bridge_covariance_equals_the_subtractive_form():
    for dt in (0.1, 0.5, 2.0):
        for J in (1, 2, 5, 9):
            for j in range(1, J + 1):
                tau = LD(j) * (LD(dt) / LD(J + 1))
                a, b = ref.qc_closed(dt, tau), ref.qc_subtractive(dt, tau)
                scale = np.sqrt(np.outer(np.diag(a), np.diag(a)))
                assert float((np.abs(a - b) / scale).max()) < 1e-15, (dt, J, j)     # long double: eps 1e-19 x cancellation
                assert a[0, 0] > 0 and a[1, 1] > 0 and a[0, 0] * a[1, 1] > a[0, 1] ** 2


def test_scalars_are_those_of_the_oracle(oracle):
    for dt, tau in ((0.5, 0.1), (0.1, 0.05), (2.0, 1.9)):
        L, P = oracle.gp_matrices(3, None, dt, tau)
        L2, P2 = ref.gp_scalars(dt, tau, np.float64)
        I = np.eye(3)
        assert np.abs(L - np.kron(L2, I)).max() < 1e-14 and np.abs(P - np.kron(P2, I)).max() < 1e-14


def test_dense_formula_equals_the_fine_chain_inverse():
    """D = 2, non-diagonal Qc, N = 3, J = 2: the intermediate states as variables of a fine GP chain, random information
    on the support states and one likelihood on an interpolated combination of a support pair.  The diagonal blocks of
    the dense inverse are Sigma(m); 1e-12 leaves 100 x for the conditioning of the inverse (measured: 1.1e-13)."""
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
    L2, P2 = ref.gp_scalars(dt, 2 * h, np.float64)            # a likelihood on a . (Lambda z_1 + Psi z_2)
    a = rng.normal(size=(1, n))
    row = np.zeros((1, Md * n))
    row[:, blk(1 * (J + 1), 0)[0]] = a @ np.kron(L2, I)
    row[:, blk(2 * (J + 1), 0)[0]] = a @ np.kron(P2, I)
    H += row.T @ row / 0.05 ** 2
    S = np.linalg.inv(H)
    sup = [i * (J + 1) for i in range(N + 1)]
    Sd = np.stack([S[blk(m, m)] for m in sup])
    So = np.stack([S[blk(sup[i + 1], sup[i])] for i in range(N)])
    cov = ref.dense_cov(Sd, So, Qc, dt, J)
    brute = np.stack([S[blk(m, m)] for m in range(Md)])
    e = ref.e_cov(brute, cov)
    print(f"dense formula against the fine-chain inverse: {e:.2e}")
    assert e < 1e-12


# ---------------------------------------------------------------------------------------------- yardstick and CAP
def _measures(c, b, cov_hat, J, truth_cov=None):
    """(e_cov, e_sig) of a float64 dense covariance of trajectory b against the long-double truth"""
    tr = post.truth(c["Hd"][b], c["Ho"][b])
    cov = ref.dense_cov(*tr, c["p"].setting.Qc, c["dt"], J) if truth_cov is None else truth_cov
    s2, sbar = ref.sigma_parts(c["geo"][b], cov, c["D"])
    s2_hat, _ = ref.sigma_parts(c["geo"][b], np.asarray(cov_hat, dtype=np.float64), c["D"])
    sig_hat = np.sqrt(np.maximum(s2_hat.astype(np.float64), 0))
    return ref.e_cov(cov_hat, cov), ref.e_sig(sig_hat, s2, sbar, c["geo"][b]["inr"]), cov


@pytest.mark.parametrize("N,J", [(1, 5), (5, 5), (16, 3), (33, 1)])
def test_float64_yardsticks_stay_below_cap_and_the_slip_does_not(oracle, N, J):
    c = solved(oracle, N, J)
    Qc = c["p"].setting.Qc
    for b in range(3):
        rec, inv = ref.band_float64(c["Hd"][b], c["Ho"][b])
        ec_r, es_r, cov = _measures(c, b, ref.dense_cov(*rec, Qc, c["dt"], J, np.float64), J)
        ec_i, es_i, _ = _measures(c, b, ref.dense_cov(*inv, Qc, c["dt"], J, np.float64), J, cov)
        print(f"N={N} J={J} trajectory {b}: e_cov recursion {ec_r:.2e}, dense inv {ec_i:.2e}; e_sig {es_r:.2e}, {es_i:.2e}")
        assert max(ec_r, ec_i) < CAP and max(es_r, es_i) < CAP
        if N >= 5:      # N = 1 does not see the slip: both of its states are pinned
            tr = post.truth(c["Hd"][b], c["Ho"][b])
            slipped = ref.dense_cov(*tr, Qc, c["dt"], J, slip=(1, 1e-6)).astype(np.float64)
            ec_s, es_s, _ = _measures(c, b, slipped, J, cov)
            print(f"    1e-6 slip in Psi_2[0][1] of checked state 1: e_cov {ec_s:.2e}, e_sig {es_s:.2e}")
            assert ec_s > CAP and es_s > CAP


# ---------------------------------------------------------------------------------------------- motivation
@pytest.mark.parametrize("N,J", [(5, 5), (16, 3), (33, 2)])
def test_the_deterministic_check_misses_the_risky_pairs(oracle, N, J):
    """every non-penetrating row has its min_clearance at checked state 0 (the pinned start), and its smallest
    clearance / sigma at another pair, below 4"""
    c = solved(oracle, N, J)
    seen = 0
    for b in range(3):
        if not c["score"]["min_clearance"][b] > 0:
            continue
        seen += 1
        assert c["score"]["worst"][b][0] == 0
        cov = ref.dense_cov(*post.truth(c["Hd"][b], c["Ho"][b]), c["p"].setting.Qc, c["dt"], J)
        s2, _ = ref.sigma_parts(c["geo"][b], cov, c["D"])
        r = ref.robust(c["geo"][b], c["radius"], s2, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(c["geo"][b]["inr"] & (r["sigma"] > 0), r["clear"] / r["sigma"], np.inf)
        m, s = np.unravel_index(np.argmin(ratio), ratio.shape)
        print(f"N={N} J={J} row {b}: min_clearance {c['score']['min_clearance'][b]:.4f} at {tuple(c['score']['worst'][b])}, "
              f"smallest clearance / sigma {float(ratio[m, s]):.2f} at ({m}, {s}); sigma {float(r['sigma'][r['sigma'] > 0].min()):.1e} .. "
              f"{float(r['sigma'].max()):.1e}")
        assert (m, s) != tuple(c["score"]["worst"][b]) and m != 0 and float(ratio[m, s]) < 4
    assert seen >= 1


# ---------------------------------------------------------------------------------------------- the C ABI, no device
def _eng():
    from gpmp2_amd import engine
    return engine.Engine()


NAMES = ("gpmp2mi_gp_interpolate_cov", "gpmp2mi_gp_interpolate_cov_dev", "gpmp2mi_risk_traj", "gpmp2mi_risk_traj_dev",
         "gpmp2mi_plan_marginals_dense", "gpmp2mi_plan_marginals_dense_dev", "gpmp2mi_plan_risk", "gpmp2mi_plan_risk_dev")


def test_entry_points_have_the_declared_signatures():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pub = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gpmp2mi.h")).read(), flags=re.S)
    pub = re.sub(r"\s+", " ", pub)
    band = ("int B, int total_step, const double* Sdiag, const double* Soff, double* cov")
    risk = ("(const gpmp2mi_robot* robot, const gpmp2mi_sdf* sdf, const double* Qc, double delta_t, int inter_step, int B, "
            "int total_step, const double* traj, const double* Sdiag, const double* Soff, const int* ok, double kappa, "
            "double* robust_clearance, int* worst, double* sigma_worst, int* out_of_range, double* sigma")
    outs = "double* robust_clearance, int* worst, double* sigma_worst, int* out_of_range, double* sigma, int* ok"
    for decl in (
        f"int gpmp2mi_gp_interpolate_cov(int dof, const double* Qc, double delta_t, int inter_step, {band});",
        f"int gpmp2mi_gp_interpolate_cov_dev(int dof, const double* Qc, double delta_t, int inter_step, {band}, void* stream);",
        f"int gpmp2mi_risk_traj{risk});",
        f"int gpmp2mi_risk_traj_dev{risk}, void* stream);",
        "int gpmp2mi_plan_marginals_dense(gpmp2mi_plan* p, int inter_step, double* cov, int* ok);",
        "int gpmp2mi_plan_marginals_dense_dev(gpmp2mi_plan* p, int inter_step, double* cov, int* ok, void* stream);",
        f"int gpmp2mi_plan_risk(gpmp2mi_plan* p, int inter_step, double kappa, {outs});",
        f"int gpmp2mi_plan_risk_dev(gpmp2mi_plan* p, int inter_step, double kappa, {outs}, void* stream);",
    ):
        assert decl in pub, decl
    assert "posterior on the executed timeline" in open(os.path.join(root, "include", "gpmp2mi.h")).read()
    lib = _eng().lib
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name


def test_bad_arguments_are_refused_before_any_device_work():
    from gpmp2_amd import engine
    lib = _eng().lib
    d = engine.dptr
    Sd, So = np.tile(np.eye(4), (1, 3, 1, 1)), np.zeros((1, 2, 4, 4))
    cov, t = np.zeros((1, 7, 4, 4)), np.zeros((1, 3, 4))
    icov = lib.gpmp2mi_gp_interpolate_cov
    good = dict(dof=2, dt=0.1, J=2, B=1, N=2)

    def interp(Sd_=Sd, So_=So, **kw):
        a = dict(good, **kw)
        return icov(a["dof"], None, a["dt"], a["J"], a["B"], a["N"], None if Sd_ is None else d(Sd_),
                    None if So_ is None else d(So_), d(cov))

    assert interp(Sd_=None) == 1 and b"null" in lib.gpmp2mi_last_error()
    assert interp(So_=None) == 1
    assert interp(J=-1) == 1 and b"inter_step" in lib.gpmp2mi_last_error()
    assert interp(B=-1) == 1 and b"B must" in lib.gpmp2mi_last_error()
    assert interp(N=0) == 1 and b"total_step" in lib.gpmp2mi_last_error()
    assert interp(dt=0.0) == 1 and interp(dt=-1.0) == 1 and b"delta_t" in lib.gpmp2mi_last_error()
    assert interp(dof=0) == 1 and interp(dof=19) == 1 and b"dof" in lib.gpmp2mi_last_error()
    assert interp(B=0) == 0                                  # B == 0 does nothing, device or not
    assert lib.gpmp2mi_gp_interpolate_cov_dev(2, None, 0.1, -1, 1, 2, 8, 8, 8, None) == 1
    assert lib.gpmp2mi_gp_interpolate_cov_dev(2, None, 0.1, 2, 1, 2, None, 8, 8, None) == 1
    # risk_traj: a handle that is never read stands in for the robot and the field -- the refusal comes first
    fake = ctypes.c_void_p(8)
    rt = lib.gpmp2mi_risk_traj

    def risk(r=fake, s=fake, traj=t, Sd_=Sd, kappa=3.0, **kw):
        a = dict(good, **kw)
        return rt(r, s, None, a["dt"], a["J"], a["B"], a["N"], None if traj is None else d(traj),
                  None if Sd_ is None else d(Sd_), d(So), None, kappa, None, None, None, None, None)

    assert risk(r=None) == 1 and risk(s=None) == 1 and risk(traj=None) == 1 and risk(Sd_=None) == 1
    assert risk(J=-1) == 1 and risk(B=-1) == 1 and risk(N=0) == 1 and risk(dt=0.0) == 1
    for bad in (-1.0, float("nan"), float("inf")):
        assert risk(kappa=bad) == 1 and b"kappa" in lib.gpmp2mi_last_error()
    assert lib.gpmp2mi_risk_traj_dev(None, fake, None, 0.1, 2, 1, 2, 8, 8, 8, None, 3.0, None, None, None, None, None,
                                     None) == 1
    assert lib.gpmp2mi_risk_traj_dev(fake, fake, None, 0.1, 2, 1, 2, 8, 8, 8, None, -3.0, None, None, None, None, None,
                                     None) == 1
    # plans
    assert lib.gpmp2mi_plan_marginals_dense(None, 2, None, None) == 1 and b"null plan" in lib.gpmp2mi_last_error()
    assert lib.gpmp2mi_plan_marginals_dense_dev(None, 2, None, None, None) == 1
    assert lib.gpmp2mi_plan_risk(None, 2, 3.0, None, None, None, None, None, None) == 1
    assert lib.gpmp2mi_plan_risk_dev(None, 2, 3.0, None, None, None, None, None, None, None) == 1
    assert lib.gpmp2mi_plan_marginals_dense(fake, -1, None, None) == 1 and b"inter_step" in lib.gpmp2mi_last_error()
    assert lib.gpmp2mi_plan_risk(fake, 2, -1.0, None, None, None, None, None, None) == 1
    assert lib.gpmp2mi_plan_risk_dev(fake, 2, float("nan"), None, None, None, None, None, None, None) == 1


def test_without_a_gpu_the_calls_say_so():
    """no quiet fall-back: GPMP2MI_ERR_NO_DEVICE without a device (with one, the same call succeeds)"""
    eng = _eng()
    Sd = np.tile(2.0 * np.eye(4), (1, 3, 1, 1))
    So = np.zeros((1, 2, 4, 4))
    if eng.device_count() == 0:
        from gpmp2_amd import engine
        with pytest.raises(engine.Gpmp2miError) as ei:
            eng.gp_interpolate_cov(2, None, 0.1, 2, Sd, So)
        assert ei.value.code == 2
    else:
        cov = eng.gp_interpolate_cov(2, None, 0.1, 2, Sd, So)
        want = ref.dense_cov(Sd[0], So[0], None, 0.1, 2)
        assert ref.e_cov(cov[0], want) < 1e-14 and np.array_equal(cov[0, ::3], Sd[0])


def test_wrappers_reject_bad_shapes_before_the_library():
    from gpmp2_amd import engine

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError(f"reached the library: {name}")

    class Rob:
        dof, S, ptr = 3, 4, None

    eng = engine.Engine.__new__(engine.Engine)
    eng.lib = NoLib()
    Sd, So = np.zeros((2, 5, 6, 6)), np.zeros((2, 4, 6, 6))
    with pytest.raises(ValueError, match="Sdiag: expected"):
        eng.gp_interpolate_cov(3, None, 0.1, 2, np.zeros((2, 5, 6, 4)), So)
    with pytest.raises(ValueError, match="Soff: expected"):
        eng.gp_interpolate_cov(3, None, 0.1, 2, Sd, np.zeros((2, 3, 6, 6)))
    with pytest.raises(ValueError, match="Qc: expected"):
        eng.gp_interpolate_cov(3, np.eye(2), 0.1, 2, Sd, So)
    with pytest.raises(ValueError, match="inter_step"):
        eng.gp_interpolate_cov(3, None, 0.1, -1, Sd, So)
    with pytest.raises(ValueError, match="delta_t"):
        eng.gp_interpolate_cov(3, None, 0.0, 1, Sd, So)
    with pytest.raises(ValueError, match="traj: expected"):
        eng.risk_traj(Rob(), Rob(), None, 0.1, 2, np.zeros((2, 4, 6)), Sd, So, 3.0)
    with pytest.raises(ValueError, match="kappa"):
        eng.risk_traj(Rob(), Rob(), None, 0.1, 2, np.zeros((2, 5, 6)), Sd, So, -1.0)
    with pytest.raises(ValueError, match="ok: expected"):
        eng.risk_traj(Rob(), Rob(), None, 0.1, 2, np.zeros((2, 5, 6)), Sd, So, 3.0, ok=np.ones(3))
    pl = engine.Plan.__new__(engine.Plan)
    pl.eng, pl.B, pl.D, pl.N, pl.h, pl.robot = eng, 2, 3, 4, None, Rob()
    with pytest.raises(ValueError, match="inter_step"):
        pl.marginals_dense(-1)
    with pytest.raises(ValueError, match="kappa"):
        pl.risk(2, float("nan"))
    with pytest.raises(ValueError, match="kappa"):
        pl.risk_dev(2, -0.5)

    class Tensor:                      # what _dev_arg reads of a torch tensor
        dtype, shape = "torch.float64", (2, 9, 6, 6)

        class device:
            type = "cuda"

        def is_contiguous(self):
            return True

        def data_ptr(self):
            return 8

    with pytest.raises(ValueError, match="cov: expected"):
        pl.marginals_dense_dev(2, cov=Tensor())          # Md = 13 for inter_step = 2
    with pytest.raises(ValueError, match="sigma: expected"):
        pl.risk_dev(2, 3.0, sigma=Tensor())
